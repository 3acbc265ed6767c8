"""Convergence of the fog march in the number of steps, with and without the Bayer jitter (a script, not a test).

    python tests/fog_quality.py [--size 1920x1080] [--shadow-dim 2048] [--density 0.02]

The checker (tests/fog_ref) on the reference scene's depth plane and rendered cascades (crychic_renderer_amd.scene on the CPU) over a
uniform mid-grey frame, so that every difference is the fog's: the mean absolute RGBA8 difference of N = 4, 8, 16, 32 against N = 64,
once with the definition's jitter and once with jit = 0.5 for every pixel (the checker's `jitter` switch; never the definition).  The
reference frame of each column is N = 64 of the same column.  Also each jittered N against the unjittered N = 64.  Prints one JSON
line."""
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
    ap.add_argument("--shadow-dim", type=int, default=2048)
    ap.add_argument("--density", type=float, default=0.02)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    import fog_lib as fg
    from crychic_renderer_amd import scene
    planes = scene.make_scene(W, H, shadow_dim=a.shadow_dim, cube_dim=8, device="cpu")
    frame = fg.Frame.from_pass_cb(planes["consts"].pass_cb, planes["depth"].numpy().view(np.uint32), planes["shadow"].numpy().view(np.uint32))
    img = np.full((H, W, 4), 128, np.uint8)

    def run(n, jitter):
        return fg.checker(frame, img, dict(fg.DEFAULTS, density=a.density, steps=n), jitter=jitter)[0].astype(np.int32)
    out = {"metric": "fog_convergence", "frame": [W, H], "shadow_dim": a.shadow_dim, "density": a.density}
    ref = {j: run(64, j) for j in (True, False)}
    for jitter in (True, False):
        tag = "jitter" if jitter else "no_jitter"
        for n in (4, 8, 16, 32):
            got = run(n, jitter)
            out["mae_n%d_%s" % (n, tag)] = round(float(np.abs(got - ref[jitter]).mean()), 5)
            out["max_n%d_%s" % (n, tag)] = int(np.abs(got - ref[jitter]).max())
            if jitter:
                out["mae_n%d_jitter_vs_plain64" % n] = round(float(np.abs(got - ref[False]).mean()), 5)
    out["mae_64_jitter_vs_plain64"] = round(float(np.abs(ref[True] - ref[False]).mean()), 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
