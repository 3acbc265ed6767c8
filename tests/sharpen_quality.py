"""What the sharpening pass does to the picture behind the temporal passes, and what sets its default strength (recorded in
profiles/sharpen_quality.txt, README.md and DESIGN.md section 32, not a test):

    python tests/sharpen_quality.py [--render 640x360] [--display 960x540] [--frames 16] [--shadow-dim 1024] [--limit 3072]

The still reference scene lit by the CPU oracle as tests/taa_upscale_quality.py sets it up.  First leg: --frames jittered frames at
--render accumulated at --display by the checker of crychic_taa_upscale, then the checker of crychic_sharpen (tests/sharpen_ref: the
definition the device reproduces byte for byte) at strength 0, 32, .., 256.  Second leg: the same sweep behind --frames jittered
--display frames under crychic_taa's checker at its defaults.  The truth is the scene at four times --display box-filtered 4 x 4.
Prints one JSON line: for each leg and strength the mean absolute RGB error over all pixels and over the edge pixels (those where the
native --display frame differs from the truth), and `default_strength` by the rule: the sampled strength with the lowest all-pixel
error on the upsampled leg, provided its edge-pixel error is below that of strength 0; otherwise 0."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

STRENGTHS = tuple(range(0, 257, 32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--render", default="640x360")
    ap.add_argument("--display", default="960x540")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--shadow-dim", type=int, default=1024)
    ap.add_argument("--limit", type=int, default=None, help="default: the pass's")
    a = ap.parse_args()
    Wi, Hi = (int(v) for v in a.render.lower().split("x"))
    Wo, Ho = (int(v) for v in a.display.lower().split("x"))
    import sharpen_lib as sl
    import taa_lib as ta
    import taa_upscale_lib as tu
    limit = sl.DEFAULT_LIMIT if a.limit is None else a.limit
    small = ta.StillScene(Wi, Hi, shadow_dim=a.shadow_dim)
    hist, up = None, None
    for k in range(a.frames):
        jit = ta.jitter(k)
        lit, depth, ivp = small.frame(jit)
        up, hist, _ = tu.checker(tu.Case("still%d" % k, ivp, small.cur, small.cur, jit, depth, lit, (Wo, Ho), hist, tu.DEFAULT_BLEND, tu.RESET if hist is None else 0))
    native_scene = ta.StillScene(Wo, Ho, shadow_dim=a.shadow_dim)
    native = native_scene.frame()[0]
    native_taa = native_scene.resolve(a.frames)
    truth = ta.box_filter(ta.StillScene(4 * Wo, 4 * Ho, shadow_dim=a.shadow_dim).frame()[0], 4)[..., :3]
    edge = (native[..., :3].astype(np.int32) != truth).any(-1)

    def mae(img, mask=None):
        e = np.abs(img[..., :3].astype(np.int32) - truth)
        return round(float((e if mask is None else e[mask]).mean()), 5)
    out = {"render": [Wi, Hi], "display": [Wo, Ho], "frames": a.frames, "limit": limit, "shadow_dim": a.shadow_dim,
           "truth": "%dx%d box-filtered 4x4" % (4 * Wo, 4 * Ho), "edge_pixels_share": round(float(edge.mean()), 6),
           "mae_all_native": mae(native), "mae_edge_native": mae(native, edge), "strengths": list(STRENGTHS)}
    for name, img in (("upscaled", up), ("native_taa", native_taa)):
        sharp = [sl.checker(img, s, limit) for s in STRENGTHS]
        assert np.array_equal(sharp[0], img), "strength 0 is not the identity"
        out["mae_all_" + name] = [mae(f) for f in sharp]
        out["mae_edge_" + name] = [mae(f, edge) for f in sharp]
    allp, edgep = out["mae_all_upscaled"], out["mae_edge_upscaled"]
    best = min(range(len(STRENGTHS)), key=lambda k: (allp[k], k))
    out["default_strength"] = STRENGTHS[best] if best and edgep[best] < edgep[0] else 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
