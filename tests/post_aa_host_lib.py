"""Builds and loads tests/post_aa_host (TEST INFRASTRUCTURE ONLY): csrc/post_aa_core.hpp, the body of post_aa_kernel, compiled for the
host.  With CRYCHIC_SANITIZE=1 (tools/sanitize.sh) it is the ASan + UBSan build."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import CLANG, CSRC, ROOT, SANITIZE, build_sanitized
from post_aa_lib import params_array

DIR = os.path.join(ROOT, "tests", "post_aa_host")
SRC, LIB = os.path.join(DIR, "post_aa_host.cpp"), os.path.join(DIR, "libpostaahost.so")
AUTO, VECTOR, SCALAR = 0, 1, 2


def build():
    if SANITIZE:
        return build_sanitized("libpostaahost.so", [SRC])
    deps = [SRC, os.path.join(CSRC, "post_aa_core.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.run([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", LIB], check=True)
    return LIB


_LIB = None


def antialias(src, out, params=None, row0=0, rows=None, path=AUTO):
    """Rows [row0, row0 + rows) of `out` from `src` (both (H, W, 4) uint8, contiguous, used in place) as the kernel body writes them.
    path: AUTO = the launcher's choice, VECTOR / SCALAR = that path.  Returns the path taken, or -1 where VECTOR is not possible."""
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.pah_antialias.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]
    H, W = src.shape[:2]
    assert src.flags.c_contiguous and out.flags.c_contiguous and src.dtype == out.dtype == np.uint8 and out.shape == src.shape
    p = params_array(params)
    return _LIB.pah_antialias(src.ctypes.data, out.ctypes.data, W, H, row0, H - row0 if rows is None else rows, p.ctypes.data, path)
