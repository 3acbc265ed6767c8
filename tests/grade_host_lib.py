"""Builds and loads tests/grade_host (TEST INFRASTRUCTURE ONLY): csrc/grade_core.hpp, the body of the colour grade kernel and the
table builder, compiled for the host with the workgroups, the LDS array and the barrier emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim

DIR = os.path.join(ROOT, "tests", "grade_host")
SRC, LIB = os.path.join(DIR, "grade_host.cpp"), os.path.join(DIR, "libgradehost.so")
STATS = ("groups", "vec_launches")


def build():
    return build_host_shim(SRC, LIB, ("grade_core.hpp", "devmath.hpp", "gamma_pow.inc"))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.gh_grade.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        _LIB.gh_grade.restype = None
        _LIB.gh_div255_mismatches.restype = C.c_uint32
        _LIB.gh_build_lut.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        _LIB.gh_build_lut.restype = None
    return _LIB


def grade(src, out, lut, row0=0, rows=None, cus=3):
    """The kernel's body over `src` and `out` ((H, W, 4) uint8, contiguous, used in place; the same array: in place) through the
    (N, N, N, 4) table `lut`, planned for `cus` compute units.  Returns {stat: count}."""
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype == np.uint8 and out.shape == src.shape
    lut = np.ascontiguousarray(lut, np.uint8)
    stats = np.zeros(len(STATS), np.uint32)
    _lib().gh_grade(src.ctypes.data, out.ctypes.data, W, H, row0, H - row0 if rows is None else rows, lut.ctypes.data, lut.shape[0], cus,
                    stats.ctypes.data)
    return dict(zip(STATS, (int(v) for v in stats)))


def div255_mismatches():
    return int(_lib().gh_div255_mismatches())


def build_lut(params, N):
    """The builder's body for the ten floats `params` (slope, offset, power, saturation): an (N, N, N, 4) uint8 table."""
    p = np.asarray(params, np.float32)
    assert p.shape == (10,)
    lut = np.zeros((N, N, N, 4), np.uint8)
    _lib().gh_build_lut(p.ctypes.data, N, lut.ctypes.data)
    return lut
