"""Builds and loads tests/decal_host (TEST INFRASTRUCTURE ONLY): csrc/decal_core.hpp, the body of decal_kernel, compiled for the host
with the workgroup walk, the wavefront's box reduction, lane k's test of decal k, the vote and the mask walk emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import decal_lib

DIR = os.path.join(ROOT, "tests", "decal_host")
SRC, LIB = os.path.join(DIR, "decal_host.cpp"), os.path.join(DIR, "libdecalhost.so")


def build():
    return build_host_shim(SRC, LIB, ("decal_core.hpp", "light_core.hpp", "devmath.hpp", "gamma_pow.inc"), api_header=True)


_LIB = None


def tile_grid(W, rows):
    """(bands, tiles per band) of the mask array a call over `rows` rows of a W-wide frame fills: 8 x 8 tiles, four per workgroup."""
    return (rows + 7) // 8, 4 * ((W + 31) // 32)


def apply(frame, mix, decals, textures, planes, row0=0, rows=None, masks=False):
    """Rows [row0, row0 + rows) of `planes` ([g0, g1, g2] uint8 arrays in the formats of `mix`, modified in place) as the kernel body
    writes them.  Returns the number of workgroups walked; with masks=True also the (bands, tiles) uint64 array of the tiles' masks."""
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.dch_apply.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p]
        _LIB.dch_apply.restype = C.c_uint32
    H, W = frame.H, frame.W
    rows = H - row0 if rows is None else rows
    decals = np.ascontiguousarray(decals)
    tex = decal_lib.ref_textures(textures)         # crychic_texture has the checker's layout
    m = np.zeros(tile_grid(W, rows), np.uint64) if masks else None
    groups = _LIB.dch_apply(frame.view.ctypes.data, frame.proj.ctypes.data, frame.depth.ctypes.data, planes[0].ctypes.data, planes[1].ctypes.data,
                            planes[2].ctypes.data, decal_lib.MIXES[mix], decals.ctypes.data if len(decals) else None, len(decals), C.addressof(tex),
                            len(textures), W, H, row0, rows, None if m is None else m.ctypes.data)
    return (groups, m) if masks else groups
