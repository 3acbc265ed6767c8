"""Builds and loads the checker and the host harness of the prefiltered cube map chain and the glossy reflection lookup (TEST
INFRASTRUCTURE ONLY): tests/gloss_ref/libglossref.so -- tests/point_shadow_ref/point_shadow_ref.c included unchanged, with a sample
table of its own, the prefilter and the lighting pixel restated with the gloss lookup, built with the oracle's flags -- and
tests/gloss_host/libglosshost.so, csrc/cube_prefilter_core.hpp and the gloss lighting call (tests/hostsim/host_light.hpp, bound through
light_bind.hpp) compiled for the host.  Both are rebuilt when a source is newer.  With CRYCHIC_SANITIZE=1 the harness is the ASan +
UBSan build."""
import ctypes as C
import os

import numpy as np

import local_light_lib
import point_shadow_lib
import hostsim_lib
from hostsim_lib import LIGHT_ARGTYPES, ROOT, run_light

GLOSS = 0x800       # CRYCHIC_LIGHT_CUBE_GLOSS

REF_DIR, HOST_DIR = os.path.join(ROOT, "tests", "gloss_ref"), os.path.join(ROOT, "tests", "gloss_host")
REF_SRC, REF_LIB = os.path.join(REF_DIR, "gloss_ref.c"), os.path.join(REF_DIR, "libglossref.so")
HOST_SRC, HOST_LIB = os.path.join(HOST_DIR, "gloss_host.cpp"), os.path.join(HOST_DIR, "libglosshost.so")


class Table(C.Structure):
    """cry::CubePrefilterTable / gl_table"""
    _fields_ = [("s", C.c_float * 4 * 32), ("count", C.c_uint32), ("rcpW", C.c_float)]


def build_ref():
    return local_light_lib.build_checker(REF_LIB, [REF_SRC, point_shadow_lib.REF_SRC, local_light_lib.REF_SRC])


def build_host():
    return hostsim_lib.build_host(HOST_LIB, HOST_SRC, ("cube_prefilter_core.hpp",))


def build():
    return build_ref(), build_host()


def chain_bytes(dim, levels):
    return sum(6 * 4 * max(dim >> k, 1) ** 2 for k in range(levels))


def level_view(chain, dim, k):
    """Level k of a flat chain as a (6, d, d, 4) view."""
    d = max(dim >> k, 1)
    off = chain_bytes(dim, k)
    return chain[off:off + 6 * d * d * 4].reshape(6, d, d, 4)


class GlossLib:
    def __init__(self):
        ref, host = build()
        self._ref, self._host = C.CDLL(ref), C.CDLL(host)
        vp, u32 = C.c_void_p, C.c_uint32
        self._ref.gl_prefilter_samples.argtypes = [u32, u32, u32, vp, C.POINTER(u32), C.POINTER(C.c_float)]
        self._ref.gl_prefilter_chain.argtypes = [vp, vp, u32, u32]
        self._ref.gl_prefilter_chain.restype = None
        self._host.gh_prefilter.argtypes = [vp, vp, u32, u32, vp]
        self._host.gh_prefilter.restype = None
        self._ref.gl_deferred_light_gloss.argtypes = LIGHT_ARGTYPES
        self._host.gh_light.argtypes = LIGHT_ARGTYPES

    def samples(self, dim, levels, level):
        """The checker's table of a level: (the 32 x 4 float32 array, entries past the count zero; count; rcpW), or None if refused."""
        s = np.zeros((32, 4), np.float32)
        n, r = C.c_uint32(), C.c_float()
        if self._ref.gl_prefilter_samples(dim, levels, level, s.ctypes.data, C.byref(n), C.byref(r)) != 0:
            return None
        return s, n.value, np.float32(r.value)

    def prefilter(self, chain, dim, levels):
        """The checker's prefiltered chain of the flat uint8 chain `chain`."""
        src = np.ascontiguousarray(chain[:chain_bytes(dim, levels)], np.uint8)
        dst = np.zeros_like(src)
        self._ref.gl_prefilter_chain(src.ctypes.data, dst.ctypes.data, dim, levels)
        return dst

    def checker_light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights):
        """The checker's gloss frame (RGBA8, radiance): point_shadow_lib's checker arguments; flags carries CRYCHIC_LIGHT_CUBE_GLOSS and
        CRYCHIC_LIGHT_CUBE_LEVELS(n), p["cube"] the flat chain and cube_dim its face size; float32 planes."""
        return run_light(self._ref.gl_deferred_light_gloss, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def host_light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights):
        """The same call through the kernel body on the host (tests/gloss_host gh_light); formats=True: planes in their own dtypes."""
        return run_light(self._host.gh_light, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def host_prefilter(self, chain, dim, levels, guard=64):
        """The kernel body's prefiltered chain on the host, with the product's tables; `guard` bytes of 0xA5 follow the chain."""
        from crychic_renderer_amd import lib
        from crychic_renderer_amd._lib import check
        n = chain_bytes(dim, levels)
        src = np.ascontiguousarray(chain[:n], np.uint8)
        dst = np.full(n + guard, 0xA5, np.uint8)
        tables = (Table * max(levels - 1, 1))()
        for k in range(1, levels):
            t, cnt, rw = tables[k - 1], C.c_uint32(), C.c_float()
            check(lib.crychic_cube_prefilter_samples(dim, levels, k, C.cast(t.s, C.c_void_p), C.byref(cnt), C.byref(rw)))
            t.count, t.rcpW = cnt.value, rw.value
        self._host.gh_prefilter(src.ctypes.data, dst.ctypes.data, dim, levels, C.addressof(tables))
        return dst, n


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = GlossLib()
    return _LIB
