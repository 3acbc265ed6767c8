"""Builds and loads tests/ssr_gloss_host (TEST INFRASTRUCTURE ONLY): csrc/ssr_pyramid_core.hpp and csrc/ssr_gloss_core.hpp, the bodies
of ssr_pyramid_kernel and ssr_gloss_kernel, compiled for the host with the workgroup and lane walks emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import ssr_lib
import ssr_gloss_lib as gl

DIR = os.path.join(ROOT, "tests", "ssr_gloss_host")
SRC, LIB = os.path.join(DIR, "ssr_gloss_host.cpp"), os.path.join(DIR, "libssrglosshost.so")
HEADERS = ("ssr_gloss_core.hpp", "ssr_pyramid_core.hpp", "ssr_core.hpp", "fog_core.hpp", "light_core.hpp", "devmath.hpp", "gamma_pow.inc")


def build():
    return build_host_shim(SRC, LIB, HEADERS, api_header=True)


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.ssgh_pyramid.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p]
        _LIB.ssgh_pyramid.restype = C.c_uint32
        _LIB.ssgh_glossy.argtypes = [C.c_void_p] * 12 + [C.c_uint32] * 5 + [C.c_void_p] * 2
        _LIB.ssgh_glossy.restype = C.c_uint32
    return _LIB


def pyramid(src, levels, workspace):
    """Levels 1 .. n_eff of the (H, W, 4) uint8 frame `src` into the flat uint8 array `workspace` (16-byte aligned, used in place) as
    the kernel body writes them.  Returns the number of workgroups walked."""
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and src.dtype == workspace.dtype == np.uint8 and workspace.ctypes.data % 16 == 0
    assert workspace.nbytes >= gl.plan(W, H, levels)[2]
    return _lib().ssgh_pyramid(src.ctypes.data, W, H, levels, workspace.ctypes.data)


def glossy(frame, src, pyr, out, params=None, gloss=None, row0=0, rows=None, mix=0):
    """Rows [row0, row0 + rows) of `out` from `src` and its pyramid `pyr` as the kernel body writes them (ssr_host_lib.ssr with the
    glossy hit colour).  Returns the number of workgroups walked."""
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype == np.uint8 and out.shape == src.shape
    assert not np.shares_memory(src, out) and frame.depth.shape == (H, W) and pyr.ctypes.data % 16 == 0
    g = [frame.plane(k, mix) for k in range(3)]
    p, q = ssr_lib.params_array(params), gl.gloss_array(gloss)
    return _lib().ssgh_glossy(frame.proj.ctypes.data, frame.vp.ctypes.data, frame.ivp.ctypes.data, frame.eye.ctypes.data, frame.nearZ.ctypes.data,
                              g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, frame.depth.ctypes.data, src.ctypes.data, pyr.ctypes.data,
                              out.ctypes.data, W, H, row0, H - row0 if rows is None else rows, ssr_lib.format_flags(mix), p.ctypes.data,
                              q.ctypes.data)
