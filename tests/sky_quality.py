"""Measures what the step counts of crychic_render_sky cost in accuracy (TEST INFRASTRUCTURE ONLY; no assertion): the RGBA8 difference
of viewSteps x sunSteps = 4x4, 8x4, 16x8 and 32x8 against 64x32 at dim 64 under four suns, for the definition's quadratic sample
spacing and for a uniform one (tests/sky_restate.py, float64, rounded to bytes); and the quadrature error of crychic_sky_sun_colour
for a sun at the zenith against the closed form, which tests/test_sky_host.py asserts at twice the value recorded here.

    python tests/sky_quality.py > profiles/sky_quality.txt"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sky_lib          # noqa: E402
import sky_restate      # noqa: E402

PAIRS = ((4, 4), (8, 4), (16, 8), (32, 8))
SUNS = (60, 20, 3, -3)
DIM = 64


def cube_bytes(el, v, s, spacing):
    value, eps, risky = sky_restate.restate(DIM, dict(sunDir=sky_lib.sun_at(el), viewSteps=v, sunSteps=s), spacing=spacing)
    return sky_restate.classify(value, eps, risky)[0].astype(np.int32)


def zenith_error(sun_steps):
    """The largest relative error over the channels of the checker's sun colour for a sun at the zenith, altitude 0, against
    sunIntensity exp(-(betaR 8 + 1.1 betaM 1.2))."""
    p = dict(sunDir=(0.0, 1.0, 0.0), altitude=0.0, sunSteps=sun_steps)
    got = sky_lib.sun_colour(p).astype(np.float64)
    want = sky_lib.DEFAULTS["sunIntensity"] * np.exp(-(sky_restate.BETA_R * 8.0 + 1.1 * sky_restate.BETA_M * 1.2))
    return float(np.max(np.abs(got - want) / want))


def main():
    print("# crychic_render_sky: RGB8 difference against 64 x 32 steps, dim %d, all six faces (tests/sky_quality.py)" % DIM)
    print("# spacing   sun_elevation  view x sun   mean_abs_diff  max_abs_diff")
    for spacing in ("quadratic", "uniform"):
        for el in SUNS:
            ref = cube_bytes(el, 64, 32, spacing)
            for v, s in PAIRS:
                d = np.abs(cube_bytes(el, v, s, spacing) - ref)
                print("%-10s  %4d           %2d x %-2d      %8.3f       %4d" % (spacing, el, v, s, d.mean(), d.max()))
    print("# the two spacings' own 64 x 32 cubes against each other")
    for el in SUNS:
        d = np.abs(cube_bytes(el, 64, 32, "quadratic") - cube_bytes(el, 64, 32, "uniform"))
        print("%-10s  %4d           64 x 32      %8.3f       %4d" % ("quad-unif", el, d.mean(), d.max()))
    print("# crychic_sky_sun_colour, sun at the zenith, altitude 0: largest relative error of a channel against the closed form")
    for n in (4, 8, 16, 32):
        print("sunSteps %2d   %.3e" % (n, zenith_error(n)))


if __name__ == "__main__":
    main()
