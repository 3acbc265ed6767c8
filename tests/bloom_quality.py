"""What the bloom pass does to the reference scene at its defaults (a script, not a test).

    python tests/bloom_quality.py [--size 1920x1080] [--thresholds 192,160,128]

The synthetic reference scene on the CPU (crychic_renderer_amd.scene's ray caster; the host build of the lighting kernel with three
directional lights, the sky fill and no ambient occlusion), then the checker (tests/bloom_ref) over that frame at the default
parameters and at each further threshold.  Reports the share of texels over the threshold (w > 0) and at full weight (w = 256), the
share of pixels the pass changes, the share of channels it saturates, and the mean absolute RGBA8 change over the whole frame and over
the changed pixels.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--thresholds", default="192,160,128")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.lower().split("x"))
    import bloom_lib as bl
    import hostsim_lib
    import scene_util
    pl = scene_util.cpu_scene(W, H, 256, 32)
    img, _ = hostsim_lib.load().light_frame(pl["consts"].pass_cb, scene_util.np_planes(pl), None, 3, 0.0, 1)
    img = np.ascontiguousarray(img)
    out = {"metric": "bloom_quality", "frame": [W, H], "defaults": bl.DEFAULTS, "thresholds": {}}
    for T in (int(v) for v in args.thresholds.split(",")):
        got, _, n = bl.checker(img, dict(threshold=T))
        diff = np.abs(got.astype(np.int32) - img.astype(np.int32))
        changed = diff.any(-1)
        out["thresholds"][str(T)] = {
            "over_threshold_share": round((n["w_interior"] + n["w_full"]) / (W * H), 6),
            "full_weight_share": round(n["w_full"] / (W * H), 6),
            "pixels_changed_share": round(float(changed.mean()), 6),
            "channels_saturated_share": round(n["saturated"] / (3 * W * H), 6),
            "mean_abs_change": round(float(diff.mean()), 4),
            "mean_abs_change_of_changed": round(float(diff[changed].mean()), 4) if changed.any() else 0.0,
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
