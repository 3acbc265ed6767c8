"""Builds and loads tests/dof_host (TEST INFRASTRUCTURE ONLY): csrc/dof_core.hpp, the body of dof_kernel, compiled for the host with
the workgroup, the LDS window, the barrier and the lane walk emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import dof_lib

DIR = os.path.join(ROOT, "tests", "dof_host")
SRC, LIB = os.path.join(DIR, "dof_host.cpp"), os.path.join(DIR, "libdofhost.so")


def build():
    return build_host_shim(SRC, LIB, ("dof_core.hpp", "devmath.hpp", "gamma_pow.inc"))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.dfh_dof.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_void_p]
        _LIB.dfh_dof.restype = C.c_uint32
        _LIB.dfh_tap.argtypes = _LIB.dfh_disc.argtypes = [C.c_uint32]
        _LIB.dfh_tap.restype = _LIB.dfh_disc.restype = C.c_uint32
    return _LIB


def params_array(params=None):
    p = dict(dof_lib.DEFAULTS, **(params or {}))
    f = np.array([p["focus"], p["aperture"]], np.float32).view(np.uint32)
    return np.array([f[0], f[1], p["radius"]], np.uint32)


def dof(frame, src, out, params=None, row0=0, rows=None):
    """Rows [row0, row0 + rows) of `out` from `src` (both (H, W, 4) uint8, contiguous, used in place) as the kernel body writes them
    for the dof_lib.Frame `frame`.  Returns the number of workgroups walked."""
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype == np.uint8 and out.shape == src.shape
    assert frame.depth.shape == (H, W)
    p, proj = params_array(params), frame.proj()
    return _lib().dfh_dof(proj.ctypes.data, frame.depth.ctypes.data, src.ctypes.data, out.ctypes.data, W, H, row0, H - row0 if rows is None else rows,
                          p.ctypes.data)


def taps():
    """[(d16, ox, oy)] in the kernel's order (197 entries), the sentinel behind them, and the disc sizes at R = 0 .. 8."""
    lib = _lib()
    e = [lib.dfh_tap(i) for i in range(198)]
    return [(v >> 16, (v & 255) - 8, ((v >> 8) & 255) - 8) for v in e[:197]], e[197], [lib.dfh_disc(R) for R in range(9)]
