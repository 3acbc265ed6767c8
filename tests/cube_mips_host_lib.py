"""Builds and loads tests/cube_mips_host (TEST INFRASTRUCTURE ONLY): csrc/cube_mips_core.hpp, the body of cube_mips_kernel, compiled
for the host.  With CRYCHIC_SANITIZE=1 (tools/sanitize.sh) it is the ASan + UBSan build."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import CLANG, CSRC, ROOT, SANITIZE, build_sanitized

DIR = os.path.join(ROOT, "tests", "cube_mips_host")
SRC, LIB = os.path.join(DIR, "cube_mips_host.cpp"), os.path.join(DIR, "libcubemipshost.so")


def build():
    if SANITIZE:
        return build_sanitized("libcubemipshost.so", [SRC])
    deps = [SRC, os.path.join(CSRC, "cube_mips_core.hpp")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.run([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", LIB], check=True)
    return LIB


def generate(cube, levels, misalign=0):
    """The chain of the 6 x dim x dim x 4 uint8 cube map `cube`, `levels` levels, as the kernel body builds it; bytes past the chain
    come back as 0xA5.  misalign: the chain starts that many bytes (a multiple of 4) past a 16-byte boundary."""
    lib = C.CDLL(build())
    lib.cmh_generate.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    dim = cube.shape[1]
    n = sum(6 * 4 * max(dim >> k, 1) ** 2 for k in range(levels))
    raw = np.full(n + 64 + 32, 0xA5, np.uint8)
    off = (-raw.ctypes.data) % 16 + misalign
    buf = raw[off:off + n + 64]
    buf[:cube.size] = cube.reshape(-1)
    lib.cmh_generate(buf.ctypes.data, dim, levels)
    return buf, n
