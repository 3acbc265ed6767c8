"""What the post-process anti-aliasing pass does to the picture (recorded in README.md and DESIGN.md section 19, not a test):

    python tests/post_aa_quality.py [--size 1920x1080] [--subpix 0,64,128,192,256]

The reference scene lit by the CPU oracle (blurCount 3, 3 lights, sky, 4096^2 cascades, literal PCF radius) at --size, and at twice
that size box-filtered 2 x 2 (rounded mean per channel) as the supersampled ground truth.  The pass is the checker's
(tests/post_aa_ref: the definition the device reproduces byte for byte).  Prints one JSON line: the mean absolute RGBA8 error
against the truth without the pass and with it -- over all pixels and over the pixels the pass changed -- and the share of pixels
changed, for the default parameters and for each --subpix value with the other parameters at their defaults."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def lit_frame(W, H):
    import oracle_lib
    import scene_util
    from crychic_renderer_amd import lib
    pl = scene_util.cpu_scene(W, H, 4096, 256)
    p, c = scene_util.np_planes(pl), pl["consts"]
    orc = oracle_lib.load()
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    ao = orc.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)
    return orc.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], ao, p["shadow"], p["cube"], 3, lib.crychic_pcf_search_radius(4096, 1), sky=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--subpix", default="0,64,128,192,256")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    import post_aa_lib as aa
    plain = lit_frame(W, H)
    big = lit_frame(2 * W, 2 * H).astype(np.int32)
    truth = (big[0::2, 0::2] + big[0::2, 1::2] + big[1::2, 0::2] + big[1::2, 1::2] + 2) >> 2
    err_plain = np.abs(plain.astype(np.int32) - truth)

    def report(params):
        out, n = aa.checker(plain, params)
        changed = (out != plain).any(-1)
        err = np.abs(out.astype(np.int32) - truth)
        r = {"pixels_changed_share": round(float(changed.mean()), 6), "edge_pixels_share": round((n["horizontal"] + n["vertical"]) / (W * H), 6),
             "mae_all_without": round(float(err_plain.mean()), 5), "mae_all_with": round(float(err.mean()), 5)}
        if changed.any():
            r["mae_changed_without"] = round(float(err_plain[changed].mean()), 5)
            r["mae_changed_with"] = round(float(err[changed].mean()), 5)
        return r

    out = {"size": [W, H], "truth": "%dx%d box-filtered 2x2" % (2 * W, 2 * H), "default": report(None)}
    for s in (int(v) for v in a.subpix.split(",") if v != ""):
        out["subpix_%d" % s] = report(dict(subpix=s))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
