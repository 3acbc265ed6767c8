"""Builds and loads tests/sharpen_host (TEST INFRASTRUCTURE ONLY): csrc/sharpen_core.hpp, the body of the sharpening kernels, compiled
for the host with a wavefront's lanes in lockstep and the lane exchange through arrays; and the counters that hold its two division
routines to the integer division."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim

DIR = os.path.join(ROOT, "tests", "sharpen_host")
SRC, LIB = os.path.join(DIR, "sharpen_host.cpp"), os.path.join(DIR, "libsharpenhost.so")
STATS = ("groups", "wide_launches")


def build():
    return build_host_shim(SRC, LIB, ("sharpen_core.hpp", "devmath.hpp", "gamma_pow.inc"))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.sh_sharpen.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 6 + [C.c_void_p]
        _LIB.sh_sharpen.restype = None
        _LIB.sh_q12_mismatches.argtypes = [C.c_int]
        _LIB.sh_q12_mismatches.restype = C.c_uint32
        _LIB.sh_div_mismatches.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
        _LIB.sh_div_mismatches.restype = C.c_uint64
    return _LIB


def sharpen(src, out, strength, limit, row0=0, rows=None):
    """The kernels' bodies over `src` and `out` ((H, W, 4) uint8, contiguous, used in place).  Returns {stat: count}."""
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype == np.uint8 and out.shape == src.shape
    stats = np.zeros(len(STATS), np.uint32)
    _lib().sh_sharpen(src.ctypes.data, out.ctypes.data, W, H, row0, H - row0 if rows is None else rows, strength, limit, stats.ctypes.data)
    return dict(zip(STATS, (int(v) for v in stats)))


def q12_mismatches(ulps=0):
    return int(_lib().sh_q12_mismatches(ulps))


def div_mismatches(t0, t1, ulps=0):
    return int(_lib().sh_div_mismatches(t0, t1, ulps))
