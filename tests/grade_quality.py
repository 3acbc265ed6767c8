"""Which table size the colour grade needs, and how close the builder is to float64 (a script, not a test).

    python tests/grade_quality.py [--size 1920x1080]

The synthetic reference scene on the CPU (crychic_renderer_amd.scene's ray caster; the host build of the lighting kernel with three
directional lights, the sky fill and no ambient occlusion), then one non-trivial look -- the "warm" ASC CDL of the builder's tests --
three ways: through the table crychic_grade_build_lut makes at N = 17, through the one at N = 33 (the checker, tests/grade_ref), and
the CDL evaluated per pixel in float64 and rounded once.  Reports the mean and the largest absolute RGBA8 difference between each pair,
and per parameter set of tests/test_grade_host.py the share of table bytes on which the builder and its float64 restatement differ.
Prints one JSON line."""
import argparse
import ctypes as C
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
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.lower().split("x"))
    import grade_lib as gl
    import hostsim_lib
    import scene_util
    from crychic_renderer_amd import _lib
    from test_grade_host import BUILDER_SETS, cdl_float64
    pl = scene_util.cpu_scene(W, H, 256, 32)
    img, _ = hostsim_lib.load().light_frame(pl["consts"].pass_cb, scene_util.np_planes(pl), None, 3, 0.0, 1)
    img = np.ascontiguousarray(img)

    def table(p, N):
        lut = np.zeros((N, N, N, 4), np.uint8)
        q = _lib.GradeParams.default(**p)
        _lib.check(_lib.lib.crychic_grade_build_lut(C.byref(q), N, lut.ctypes.data, lut.nbytes))
        return lut

    look = BUILDER_SETS["warm"]
    graded = {N: gl.checker(img, table(look, N))[..., :3].astype(np.int64) for N in (17, 33)}
    y = [np.clip(img[..., c] / 255.0 * look["slope"][c] + look["offset"][c], 0.0, 1.0) for c in range(3)]
    z = [v ** p for v, p in zip(y, look["power"])]
    luma = 0.2126 * z[0] + 0.7152 * z[1] + 0.0722 * z[2]
    exact = np.stack([np.floor(255.0 * np.clip(look["saturation"] * (c - luma) + luma, 0.0, 1.0) + 0.5) for c in z], axis=-1).astype(np.int64)

    def pair(a, b):
        d = np.abs(a - b)
        return {"mean_abs": round(float(d.mean()), 4), "max_abs": int(d.max()), "bytes_differing_share": round(float((d > 0).mean()), 6)}

    out = {"metric": "grade_quality", "frame": [W, H], "look": look,
           "n17_vs_n33": pair(graded[17], graded[33]), "n17_vs_float64": pair(graded[17], exact), "n33_vs_float64": pair(graded[33], exact),
           "pixels_changed_by_the_look_share": round(float((graded[33] != img[..., :3]).any(-1).mean()), 6), "builder_vs_float64": {}}
    for name, p in BUILDER_SETS.items():
        for N in (17, 33):
            ref, _, _ = cdl_float64(p["slope"], p["offset"], p["power"], p["saturation"], N)
            got = table(p, N)[..., :3].astype(np.int64)
            out["builder_vs_float64"]["%s_n%d" % (name, N)] = {"bytes_differing": int((got != ref).sum()), "of": int(ref.size),
                                                              "max_abs": int(np.abs(got - ref).max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
