"""Builds and loads tests/ssr_host (TEST INFRASTRUCTURE ONLY): csrc/ssr_core.hpp, the body of ssr_kernel, compiled for the host with
the workgroup and lane walk emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import ssr_lib

DIR = os.path.join(ROOT, "tests", "ssr_host")
SRC, LIB = os.path.join(DIR, "ssr_host.cpp"), os.path.join(DIR, "libssrhost.so")
HEADERS = ("ssr_core.hpp", "fog_core.hpp", "light_core.hpp", "devmath.hpp", "gamma_pow.inc")


def build():
    return build_host_shim(SRC, LIB, HEADERS, api_header=True)


_LIB = None


def ssr(frame, src, out, params=None, row0=0, rows=None, mix=0, planes=None, depth=None):
    """Rows [row0, row0 + rows) of `out` from `src` (both (H, W, 4) uint8, contiguous, used in place) as the kernel body writes them
    for the ssr_lib.Frame `frame` under format mix `mix`; planes / depth: arrays to use in place of the frame's (the same values at
    another address).  Returns the number of workgroups walked."""
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.ssh_ssr.argtypes = [C.c_void_p] * 11 + [C.c_uint32] * 5 + [C.c_void_p]
        _LIB.ssh_ssr.restype = C.c_uint32
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype == np.uint8 and out.shape == src.shape
    assert not np.shares_memory(src, out) and frame.depth.shape == (H, W)
    g = planes if planes is not None else [frame.plane(k, mix) for k in range(3)]
    depth = frame.depth if depth is None else depth
    assert all(a.flags.c_contiguous for a in g) and depth.flags.c_contiguous
    p = ssr_lib.params_array(params)
    return _LIB.ssh_ssr(frame.proj.ctypes.data, frame.vp.ctypes.data, frame.ivp.ctypes.data, frame.eye.ctypes.data, frame.nearZ.ctypes.data,
                        g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, depth.ctypes.data, src.ctypes.data, out.ctypes.data, W, H, row0,
                        H - row0 if rows is None else rows, ssr_lib.format_flags(mix), p.ctypes.data)
