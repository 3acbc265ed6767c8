"""What temporal upsampling does to the picture (recorded in profiles/taa_upscale_quality.txt, README.md and DESIGN.md section 28, not a
test):

    python tests/taa_upscale_quality.py [--render 640x360] [--display 960x540] [--frames 16] [--shadow-dim 1024] [--blend 102]

The still reference scene lit by the CPU oracle (blurCount 3, 3 lights, sky, --shadow-dim cascades, literal PCF radius) at --render,
--frames jittered frames (crychic_taa_jitter, the _jittered constant builders, the jittered ray-caster) accumulated at --display by the
checker of crychic_taa_upscale (tests/taa_upscale_ref: the definition the device reproduces byte for byte), the first a RESET frame;
against the scene at four times --display box-filtered 4 x 4 (rounded mean per channel).  Prints one JSON line: the mean absolute RGB
error against that truth over all pixels and over the edge pixels (those where the native --display frame differs from the truth) of
the accumulated frame, of one unjittered --render frame upsampled bilinearly (the pass's RESET answer), of the native unjittered
--display frame, and of --frames jittered --display frames under crychic_taa's checker at its defaults."""
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
    ap.add_argument("--render", default="640x360")
    ap.add_argument("--display", default="960x540")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--shadow-dim", type=int, default=1024)
    ap.add_argument("--blend", type=int, default=None, help="default: the pass's")
    a = ap.parse_args()
    Wi, Hi = (int(v) for v in a.render.lower().split("x"))
    Wo, Ho = (int(v) for v in a.display.lower().split("x"))
    import taa_lib as ta
    import taa_upscale_lib as tu
    blend = tu.DEFAULT_BLEND if a.blend is None else a.blend
    small = ta.StillScene(Wi, Hi, shadow_dim=a.shadow_dim)
    hist, up = None, None
    for k in range(a.frames):
        jit = ta.jitter(k)
        lit, depth, ivp = small.frame(jit)
        up, hist, _ = tu.checker(tu.Case("still%d" % k, ivp, small.cur, small.cur, jit, depth, lit, (Wo, Ho), hist, blend, tu.RESET if hist is None else 0))
    lit, depth, ivp = small.frame()
    bilinear = tu.checker(tu.Case("bilinear", ivp, small.cur, small.cur, (0.0, 0.0), depth, lit, (Wo, Ho), None, flags=tu.RESET))[0]
    native_scene = ta.StillScene(Wo, Ho, shadow_dim=a.shadow_dim)
    native = native_scene.frame()[0]
    native_taa = native_scene.resolve(a.frames)
    truth = ta.box_filter(ta.StillScene(4 * Wo, 4 * Ho, shadow_dim=a.shadow_dim).frame()[0], 4)[..., :3]
    edge = (native[..., :3].astype(np.int32) != truth).any(-1)

    def mae(img, mask=None):
        e = np.abs(img[..., :3].astype(np.int32) - truth)
        return round(float((e if mask is None else e[mask]).mean()), 5)
    out = {"render": [Wi, Hi], "display": [Wo, Ho], "frames": a.frames, "blend": blend, "shadow_dim": a.shadow_dim,
           "truth": "%dx%d box-filtered 4x4" % (4 * Wo, 4 * Ho), "edge_pixels_share": round(float(edge.mean()), 6)}
    for name, img in (("upscaled", up), ("bilinear", bilinear), ("native", native), ("native_taa", native_taa)):
        out["mae_all_" + name], out["mae_edge_" + name] = mae(img), mae(img, edge)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
