"""What the G-buffer plane formats cost in the picture (recorded in README.md and DESIGN.md section 13, not a test):

    python tests/gbuffer_f16_quality.py [--size 1920x1080]

The reference scene lit by the CPU oracle (blurCount 3, 3 lights, sky, 4096^2 cascades, literal PCF radius) from the fp32 planes and
from the planes of `mixed` (G0 float4, G1 + G2 half4), `f16` (all half4) and G0 half4 alone, widened.  Prints one JSON line: per
format the share of RGBA8 bytes and of pixels that differ from the fp32 frame, the largest difference, and the share of bytes that
differ by more than 1."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    import gbuffer_f16_lib as gf
    import oracle_lib
    import scene_util
    from crychic_renderer_amd import lib
    pl = scene_util.cpu_scene(W, H, 4096, 256)
    p, c = scene_util.np_planes(pl), pl["consts"]
    orc = oracle_lib.load()
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    ao = orc.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)
    radius = lib.crychic_pcf_search_radius(4096, 1)

    def frame(mix):
        w = gf.widen_planes(gf.pack_planes(p, mix))
        return orc.deferred_light(pcb, w["g0"], w["g1"], w["g2"], w["depth"], ao, w["shadow"], w["cube"], 3, radius, sky=True)

    f32 = frame(0)
    out = {"size": [W, H]}
    for name, mix in (("mixed", gf.MIXED), ("f16", gf.ALL_F16), ("g0_only", gf.G0_F16)):
        d = np.abs(frame(mix).astype(int) - f32.astype(int))
        out[name] = {"bytes_differing_share": round(float((d > 0).mean()), 6), "pixels_differing_share": round(float((d > 0).any(-1).mean()), 6),
                     "max_abs_diff": int(d.max()), "bytes_differing_by_more_than_1_share": round(float((d > 1).mean()), 6)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
