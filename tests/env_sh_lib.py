"""Builds and loads the checker and the host harness of the SH9 irradiance projection and of the lighting pass's ambient term from it
(TEST INFRASTRUCTURE ONLY): tests/env_sh_ref/libenvshref.so -- tests/gloss_ref/gloss_ref.c included unchanged, with the projection
and the lighting pixel restated, built with the oracle's flags -- and tests/env_sh_host/libenvshhost.so, csrc/cube_sh_core.hpp and
the lighting call with AmbientSH (tests/hostsim/host_light.hpp, bound through light_bind.hpp) compiled for the host.  Both are rebuilt when a source is
newer.  With CRYCHIC_SANITIZE=1 the harness is the ASan + UBSan build."""
import ctypes as C
import os

import numpy as np

import gloss_lib
import local_light_lib
import point_shadow_lib
import hostsim_lib
from hostsim_lib import LIGHT_ARGTYPES, ROOT, run_light

AMBIENT_SH = 0x8000     # CRYCHIC_LIGHT_AMBIENT_SH
TAIL_BYTES = 512        # CRYCHIC_CUBE_SH_BYTES
K = np.array([1, 2, 2, 2, 15 / 4, 15 / 4, 5 / 16, 15 / 4, 15 / 16], np.float64)

REF_DIR, HOST_DIR = os.path.join(ROOT, "tests", "env_sh_ref"), os.path.join(ROOT, "tests", "env_sh_host")
REF_SRC, REF_LIB = os.path.join(REF_DIR, "env_sh_ref.c"), os.path.join(REF_DIR, "libenvshref.so")
HOST_SRC, HOST_LIB = os.path.join(HOST_DIR, "env_sh_host.cpp"), os.path.join(HOST_DIR, "libenvshhost.so")


def build_ref():
    return local_light_lib.build_checker(REF_LIB, [REF_SRC, gloss_lib.REF_SRC, point_shadow_lib.REF_SRC, local_light_lib.REF_SRC])


def build_host():
    return hostsim_lib.build_host(HOST_LIB, HOST_SRC, ("cube_sh_core.hpp", "cube_prefilter_core.hpp"))


def build():
    return build_ref(), build_host()


def chain_bytes(dim, levels):
    return gloss_lib.chain_bytes(dim, max(levels, 1))


def tail_offset(dim, levels):
    """crychic_cube_sh_offset, restated."""
    return (chain_bytes(dim, levels) + 15) // 16 * 16


def with_tail(cube, dim, levels, coeffs, fill=0xA5):
    """A flat uint8 array: the cube map (or chain) `cube`, padding to 16 bytes and an environment tail whose first 144 bytes are the
    (9, 4) or (36,) float32 `coeffs`; every other byte of padding and tail is `fill`."""
    n, off = chain_bytes(dim, levels), tail_offset(dim, levels)
    out = np.full(off + TAIL_BYTES, fill, np.uint8)
    out[:n] = np.ascontiguousarray(cube, np.uint8).reshape(-1)[:n]
    out[off:off + 144] = np.ascontiguousarray(coeffs, np.float32).reshape(-1).view(np.uint8)
    return out


class EnvShLib:
    def __init__(self):
        ref, host = build()
        self._ref, self._host = C.CDLL(ref), C.CDLL(host)
        vp, u32 = C.c_void_p, C.c_uint32
        for fn in (self._ref.es_sums, self._host.eh_sums):
            fn.argtypes = [vp, u32, u32, u32, vp]
            fn.restype = None
        self._ref.es_coefficients.argtypes = [vp, vp]
        self._ref.es_coefficients.restype = None
        self._ref.es_project.argtypes = [vp, u32, vp]
        self._ref.es_project.restype = None
        self._ref.es_irradiance.argtypes = [vp, vp, vp]
        self._ref.es_irradiance.restype = None
        self._ref.es_tail_offset.argtypes = [u32, u32]
        self._ref.es_tail_offset.restype = C.c_size_t
        self._host.eh_project.argtypes = [vp, u32, vp, u32]
        self._host.eh_project.restype = None
        self._host.eh_tail_offset.argtypes = [u32, u32]
        self._host.eh_tail_offset.restype = C.c_uint64
        self._host.eh_check.argtypes = [u32, C.c_size_t, u32]
        self._ref.es_deferred_light_sh.argtypes = LIGHT_ARGTYPES
        self._host.eh_light.argtypes = LIGHT_ARGTYPES

    @staticmethod
    def _level(level):
        a = np.ascontiguousarray(level, np.uint8)
        assert a.ndim == 4 and a.shape[0] == 6 and a.shape[1] == a.shape[2] and a.shape[3] == 4
        return a, a.shape[1]

    def sums(self, level, first=0, last=None, host=False):
        """The 28 int64 sums of texels [first, last) of the (6, d, d, 4) level: the checker's, or (host) the kernel body's."""
        a, d = self._level(level)
        s = np.zeros(28, np.int64)
        (self._host.eh_sums if host else self._ref.es_sums)(a.ctypes.data, d, first, 6 * d * d if last is None else last, s.ctypes.data)
        return s

    def coefficients(self, sums):
        c = np.zeros((9, 4), np.float32)
        self._ref.es_coefficients(np.ascontiguousarray(sums, np.int64).ctypes.data, c.ctypes.data)
        return c

    def project(self, level):
        """The checker's (9, 4) float32 coefficient block of the level."""
        a, d = self._level(level)
        c = np.zeros((9, 4), np.float32)
        self._ref.es_project(a.ctypes.data, d, c.ctypes.data)
        return c

    def host_project(self, level, blocks=None, fill=0xFF):
        """The kernel bodies' environment tail (512 bytes, pre-filled with `fill`) of the level, the accumulate launch simulated with
        `blocks` workgroups (default: the launcher's count)."""
        a, d = self._level(level)
        blocks = min((6 * d * d + 255) // 256, 256) if blocks is None else blocks
        tail = np.full(TAIL_BYTES, fill, np.uint8)
        self._host.eh_project(a.ctypes.data, d, tail.ctypes.data, blocks)
        return tail

    def irradiance(self, coeffs, n):
        e = np.zeros(3, np.float32)
        self._ref.es_irradiance(np.ascontiguousarray(coeffs, np.float32).ctypes.data, np.ascontiguousarray(n, np.float32).ctypes.data, e.ctypes.data)
        return e

    def checker_light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights):
        """The checker's frame (RGBA8, radiance) with CRYCHIC_LIGHT_AMBIENT_SH: p["cube"] is with_tail's array; float32 planes."""
        return run_light(self._ref.es_deferred_light_sh, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def host_light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights):
        """The same call through the kernel body on the host (eh_light); formats=True: planes in their own dtypes."""
        self._host.eh_light.restype = C.c_int
        return run_light(self._host.eh_light, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def check(self, flags, cube_address, cube_dim):
        """light_bind.hpp's ambient_sh_check: 0 ok, 1 derivative-LOD chain, 2 null cube map, 3 misaligned tail."""
        return self._host.eh_check(flags, cube_address, cube_dim)


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = EnvShLib()
    return _LIB
