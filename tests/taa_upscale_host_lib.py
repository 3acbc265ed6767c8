"""Builds and loads tests/taa_upscale_host (TEST INFRASTRUCTURE ONLY): csrc/taa_upscale_core.hpp, the body of taa_upscale_kernel,
compiled for the host with the workgroup and lane walk emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import taa_upscale_lib as tu

DIR = os.path.join(ROOT, "tests", "taa_upscale_host")
SRC, LIB = os.path.join(DIR, "taa_upscale_host.cpp"), os.path.join(DIR, "libtaaupscalehost.so")


def build():
    return build_host_shim(SRC, LIB, ("taa_upscale_core.hpp", "taa_core.hpp", "devmath.hpp", "gamma_pow.inc"))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.tuh_taa_upscale.argtypes = [C.c_void_p] * 3 + [C.c_float] * 2 + [C.c_void_p] * 2 + [C.c_uint32] * 2 + [C.c_void_p] * 3 + [C.c_uint32] * 6
        _LIB.tuh_taa_upscale.restype = C.c_uint32
        _LIB.tuh_position.argtypes = [C.c_uint32] * 3 + [C.c_int32, C.c_int]
        _LIB.tuh_position.restype = C.c_int32
        _LIB.tuh_div.argtypes = [C.c_uint32] * 2
        _LIB.tuh_div.restype = C.c_uint32
    return _LIB


def position(o, Ni, No, J, narrow):
    return _lib().tuh_position(o, Ni, No, J, int(narrow))


def div(n, d):
    """n // d as the body divides by a divisor known on the host."""
    return _lib().tuh_div(n, d)


def taa_upscale(case, row0=0, rows=None, out=None, hist_out=None):
    """(out, history_out, workgroups walked): rows [row0, row0 + rows) as the kernel body writes them for the taa_upscale_lib.Case
    `case`, into planes of 0xA5 bytes by default."""
    Ho, Wo = case.Ho, case.Wo
    rows = Ho - row0 if rows is None else rows
    out = np.full((Ho, Wo, 4), tu.GUARD, np.uint8) if out is None else out
    hist_out = np.full((Ho, Wo, 4), tu.GUARD * 257, np.uint16) if hist_out is None else hist_out
    groups = _lib().tuh_taa_upscale(case.ivp.ctypes.data, case.cur.ctypes.data, case.prev.ctypes.data, case.jitter[0], case.jitter[1],
                                    case.depth.ctypes.data, case.img.ctypes.data, case.Wi, case.Hi,
                                    None if case.hist is None else case.hist.ctypes.data, hist_out.ctypes.data, out.ctypes.data, Wo, Ho, row0, rows,
                                    case.blend, case.flags)
    return out, hist_out, groups
