"""Builds and loads tests/bloom_host (TEST INFRASTRUCTURE ONLY): csrc/bloom_core.hpp, the bodies of the bloom kernels, compiled for the
host with the workgroups, the LDS arrays, the barriers and the votes emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import bloom_lib

DIR = os.path.join(ROOT, "tests", "bloom_host")
SRC, LIB = os.path.join(DIR, "bloom_host.cpp"), os.path.join(DIR, "libbloomhost.so")
STATS = ("groups", "zero_tiles", "silent_waves", "vec_composites")


def build():
    return build_host_shim(SRC, LIB, ("bloom_core.hpp", "devmath.hpp", "gamma_pow.inc"))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.bh_bloom.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 4 + [C.c_void_p] * 2 + [C.c_uint32, C.c_void_p]
        _LIB.bh_bloom.restype = None
        _LIB.bh_weight_mismatches.restype = C.c_uint32
        _LIB.bh_workspace_bytes.argtypes = [C.c_uint32] * 3
        _LIB.bh_workspace_bytes.restype = C.c_size_t
    return _LIB


def bloom(src, out, workspace, params=None, row0=0, rows=None, pyramid=True, composite=True):
    """The kernels' bodies over `src` and `out` ((H, W, 4) uint8, contiguous, used in place; the same array: in place) and the uint8
    array `workspace` (16-byte aligned): the pyramid, the composite of rows [row0, row0 + rows), or both.  Returns {stat: count}."""
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype == np.uint8 and out.shape == src.shape
    p = bloom_lib.params_array(params)
    assert workspace.ctypes.data % 16 == 0 and workspace.nbytes >= bloom_lib.level_offsets(W, H, int(p[4]))[1]
    stats = np.zeros(len(STATS), np.uint32)
    _lib().bh_bloom(src.ctypes.data, out.ctypes.data, W, H, row0, H - row0 if rows is None else rows, p.ctypes.data, workspace.ctypes.data,
                    (1 if pyramid else 0) | (2 if composite else 0), stats.ctypes.data)
    return dict(zip(STATS, (int(v) for v in stats)))


def weight_mismatches():
    return int(_lib().bh_weight_mismatches())


def workspace_bytes(W, H, levels):
    return int(_lib().bh_workspace_bytes(W, H, levels))
