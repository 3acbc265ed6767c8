"""What temporal anti-aliasing does to the picture (recorded in profiles/taa_quality.txt, README.md and DESIGN.md section 24, not a test):

    python tests/taa_quality.py [--size 960x540] [--frames 16] [--shadow-dim 1024]

The still reference scene lit by the CPU oracle (blurCount 3, 3 lights, sky, --shadow-dim cascades, literal PCF radius) at --size, and
at four times that size box-filtered 4 x 4 (rounded mean per channel) as the supersampled ground truth.  --frames jittered frames
(crychic_taa_jitter, the _jittered constant builders, the jittered ray-caster) go through the checker of crychic_taa (tests/taa_ref: the
definition the device reproduces byte for byte) at the default parameters, the first a RESET frame.  Prints one JSON line: the mean
absolute RGBA8 error against the truth over all pixels and over the edge pixels (those where the single unjittered frame differs from
the truth) of the unjittered frame, of the resolved frame, and of the unjittered frame through the post-process anti-aliasing
(tests/post_aa_ref at its defaults) for comparison."""
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
    ap.add_argument("--size", default="960x540")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--shadow-dim", type=int, default=1024)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    import post_aa_lib as aa
    import taa_lib as ta
    small = ta.StillScene(W, H, shadow_dim=a.shadow_dim)
    plain = small.frame()[0]
    resolved = small.resolve(a.frames)
    post = aa.checker(plain)[0]
    truth = ta.box_filter(ta.StillScene(4 * W, 4 * H, shadow_dim=a.shadow_dim).frame()[0], 4)
    edge = (plain.astype(np.int32) != truth).any(-1)

    def mae(img, mask=None):
        e = np.abs(img.astype(np.int32) - truth)
        return round(float((e if mask is None else e[mask]).mean()), 5)
    out = {"size": [W, H], "frames": a.frames, "shadow_dim": a.shadow_dim, "truth": "%dx%d box-filtered 4x4" % (4 * W, 4 * H),
           "edge_pixels_share": round(float(edge.mean()), 6),
           "mae_all_unjittered": mae(plain), "mae_all_taa": mae(resolved), "mae_all_post_aa": mae(post),
           "mae_edge_unjittered": mae(plain, edge), "mae_edge_taa": mae(resolved, edge), "mae_edge_post_aa": mae(post, edge),
           "pixels_changed_share_taa": round(float((resolved != plain).any(-1).mean()), 6),
           "pixels_changed_share_post_aa": round(float((post != plain).any(-1).mean()), 6)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
