"""Builds and loads tests/taa_host (TEST INFRASTRUCTURE ONLY): csrc/taa_core.hpp, the body of taa_kernel, compiled for the host with
the workgroup and lane walk emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import taa_lib

DIR = os.path.join(ROOT, "tests", "taa_host")
SRC, LIB = os.path.join(DIR, "taa_host.cpp"), os.path.join(DIR, "libtaahost.so")


def build():
    return build_host_shim(SRC, LIB, ("taa_core.hpp", "devmath.hpp", "gamma_pow.inc"))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.tah_taa.argtypes = [C.c_void_p] * 8 + [C.c_uint32] * 6
        _LIB.tah_taa.restype = C.c_uint32
        _LIB.tah_tile.argtypes = [C.POINTER(C.c_uint32)] * 2
        _LIB.tah_tile.restype = None
    return _LIB


def tile():
    """(kTaaGroupW, kTaaTile): the kernel's workgroup in pixels."""
    w, h = C.c_uint32(), C.c_uint32()
    _lib().tah_tile(C.byref(w), C.byref(h))
    return w.value, h.value


def taa(case, row0=0, rows=None, out=None, hist_out=None):
    """(out, history_out, workgroups walked): rows [row0, row0 + rows) as the kernel body writes them for the taa_lib.Case `case`, into
    planes of 0xA5 bytes by default."""
    H, W = case.H, case.W
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), taa_lib.GUARD, np.uint8) if out is None else out
    hist_out = np.full((H, W, 4), taa_lib.GUARD * 257, np.uint16) if hist_out is None else hist_out
    groups = _lib().tah_taa(case.ivp.ctypes.data, case.cur.ctypes.data, case.prev.ctypes.data, case.depth.ctypes.data, case.img.ctypes.data,
                            None if case.hist is None else case.hist.ctypes.data, hist_out.ctypes.data, out.ctypes.data, W, H, row0, rows,
                            case.blend, case.flags)
    return out, hist_out, groups
