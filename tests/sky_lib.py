"""Builds and loads tests/sky_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_render_sky and crychic_sky_sun_colour, plain C
written from the definition in include/crychic_hip.h with none of the kernel's code; and the corpus of parameter sets and face sizes
the host and the device tests share."""
import ctypes as C
import math
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "sky_ref")
SRC, LIB = os.path.join(DIR, "sky_ref.c"), os.path.join(DIR, "libskyref.so")

COUNTERS = ("ground", "sky", "disc", "lit", "blocked", "sunlit_ground", "dark_ground", "black")
# crychic_sky_params, field by field (48 bytes), and its defaults as include/crychic_hip.h states them
PARAMS_DTYPE = np.dtype([("sunDir", np.float32, 3), ("altitude", np.float32), ("sunIntensity", np.float32), ("exposure", np.float32),
                         ("sunAngularRadius", np.float32), ("groundAlbedo", np.float32), ("viewSteps", np.uint32), ("sunSteps", np.uint32),
                         ("reserved", np.uint32, 2)])
assert PARAMS_DTYPE.itemsize == 48
DEFAULTS = dict(sunDir=(0.0, 0.5, -0.8660254), altitude=0.002, sunIntensity=20.0, exposure=2.0, sunAngularRadius=0.02, groundAlbedo=0.3,
                viewSteps=16, sunSteps=8)


def sun_at(elevation_deg, azimuth_deg=0.0):
    """The direction towards a sun `elevation_deg` above the horizon, at `azimuth_deg` from -z towards +x (azimuth 0 lies in the
    plane x = 0)."""
    e, a = math.radians(elevation_deg), math.radians(azimuth_deg)
    return (math.cos(e) * math.sin(a), math.sin(e), -math.cos(e) * math.cos(a))


# the smallest face with texels on a face edge, one with an odd row length, one 8 x 8 wavefront tile, and two with partial and
# several tiles each way (a workgroup is 32 x 8 texels)
DIMS = (2, 3, 8, 33, 64)
SUNS = {"el90": sun_at(90), "el30": sun_at(30), "el5": sun_at(5), "el0": sun_at(0), "el-3": sun_at(-3), "el-30": sun_at(-30),
        "offaxis": (0.3, 0.5, -0.8)}
STEPS = {"s1x1": (1, 1), "sdef": (DEFAULTS["viewSteps"], DEFAULTS["sunSteps"]), "s64x32": (64, 32)}
ALTITUDES = (0.0, 50.0)
WIDE_DISC = 0.12        # radians: at dim 33 a texel spans about 0.06, so the disc covers several


def params_array(params=None):
    """A one-element array of PARAMS_DTYPE: DEFAULTS overridden by `params`."""
    p = dict(DEFAULTS, **(params or {}))
    a = np.zeros(1, PARAMS_DTYPE)
    for k, v in p.items():
        a[k][0] = v
    return a


def build():
    return build_checker(SRC, LIB)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.sky_ref.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        _REF.sky_ref.restype = None
        _REF.sky_ref_sun_colour.argtypes = [C.c_void_p, C.c_void_p]
        _REF.sky_ref_sun_colour.restype = None
    return _REF


def checker(dim, params=None, face0=0, faces=6, out=None):
    """(level 0 of faces [face0, face0 + faces) written into the (6, dim, dim, 4) uint8 cube `out` -- a cube of 0xA5 by default --,
    {counter: count over those faces})."""
    out = np.full((6, dim, dim, 4), GUARD, np.uint8) if out is None else out
    assert out.shape == (6, dim, dim, 4) and out.dtype == np.uint8 and out.flags.c_contiguous
    n = np.zeros(len(COUNTERS), np.uint64)
    p = params_array(params)
    _ref().sky_ref(out.ctypes.data, dim, face0, faces, p.ctypes.data, n.ctypes.data)
    return out, dict(zip(COUNTERS, (int(v) for v in n)))


def sun_colour(params=None):
    """crychic_sky_sun_colour as the checker computes it: three float32."""
    rgb = np.zeros(3, np.float32)
    p = params_array(params)
    _ref().sky_ref_sun_colour(p.ctypes.data, rgb.ctypes.data)
    return rgb


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

_CORPUS = {}


def corpus():
    """[(name, dim, params)]: every face size under every sun, the step counts and the altitudes cycling so that every size meets
    every step count and both altitudes and every sun meets both altitudes; 64 x 32 steps at dim 64 once (it is the slow one); the wide
    disc at dim 33 on the faces the sun looks at; two parameter sets off the defaults."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    cases = []
    steps = list(STEPS)
    for di, dim in enumerate(DIMS):
        for si, (sname, sun) in enumerate(SUNS.items()):
            st = steps[(di + si) % 3]
            if dim == 64:
                st = "s64x32" if sname == "el5" else ("sdef" if st == "s64x32" else st)
            alt = ALTITUDES[(di + si + si // 2) % 2]
            v, s = STEPS[st]
            cases.append(("dim%d_%s_%s_alt%g" % (dim, sname, st, alt), dim, dict(sunDir=sun, viewSteps=v, sunSteps=s, altitude=alt)))
    for sname in ("el30", "el5", "offaxis"):
        cases.append(("dim33_%s_wide_disc" % sname, 33, dict(sunDir=SUNS[sname], sunAngularRadius=WIDE_DISC)))
    cases.append(("dim33_el30_wide_disc_alt50", 33, dict(sunDir=SUNS["el30"], sunAngularRadius=WIDE_DISC, altitude=50.0)))
    cases.append(("dim8_el5_bright_unnormalised", 8, dict(sunDir=tuple(1000.0 * c for c in SUNS["el5"]), sunIntensity=400.0, exposure=0.5,
                                                       groundAlbedo=1.0, altitude=3.0, viewSteps=5, sunSteps=3)))
    cases.append(("dim8_el30_no_ground_no_disc", 8, dict(sunDir=SUNS["el30"], groundAlbedo=0.0, sunAngularRadius=0.0, viewSteps=7, sunSteps=31)))
    _CORPUS["cases"] = cases
    return cases


_EXPECTED = {}


def expected(name):
    """The checker's whole cube and counters for corpus case `name`; computed once, read-only."""
    if name not in _EXPECTED:
        case = {c[0]: c for c in corpus()}[name]
        out, n = checker(case[1], case[2])
        out.setflags(write=False)
        _EXPECTED[name] = (out, n)
    return _EXPECTED[name]
