"""Builds and loads tests/fog_host (TEST INFRASTRUCTURE ONLY): csrc/fog_core.hpp, the body of fog_kernel, compiled for the host with
the workgroup and lane walk emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import fog_lib

DIR = os.path.join(ROOT, "tests", "fog_host")
SRC, LIB = os.path.join(DIR, "fog_host.cpp"), os.path.join(DIR, "libfoghost.so")


def build():
    return build_host_shim(SRC, LIB, ("fog_core.hpp", "devmath.hpp", "gamma_pow.inc"))


_LIB = None


def fog(frame, src, out, params=None, row0=0, rows=None):
    """Rows [row0, row0 + rows) of `out` from `src` (both (H, W, 4) uint8, contiguous, used in place; the same array = in place) as the
    kernel body writes them for the fog_lib.Frame `frame`.  Returns the number of workgroups walked."""
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.fgh_fog.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p]
        _LIB.fgh_fog.restype = C.c_uint32
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype == np.uint8 and out.shape == src.shape
    assert frame.depth.shape == (H, W)
    p = fog_lib.params_array(params)
    maps = fog_lib.map_pointers(frame)
    return _LIB.fgh_fog(frame.ivp.ctypes.data, frame.eye.ctypes.data, frame.st.ctypes.data, frame.depth.ctypes.data, maps, frame.dim, src.ctypes.data,
                        out.ctypes.data, W, H, row0, H - row0 if rows is None else rows, p.ctypes.data)
