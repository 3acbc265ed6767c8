"""Builds and loads the local-light test harness (TEST INFRASTRUCTURE ONLY): tests/local_light_ref/liblocallightref.so, the checker
(the frozen oracle's or_light.c with the spot loop and a shadow factor per spot light, built with the oracle's flags), and
tests/local_light_ref/liblocallighthost.so, the product's local-light kernel body compiled for the host (as tests/hostsim does for
the other bodies).  Both are rebuilt when a source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "local_light_ref")
ORACLE = os.path.join(ROOT, "oracle")
CSRC = os.path.join(ROOT, "crychic_renderer_amd", "csrc")
REF_SRC, REF_LIB = os.path.join(DIR, "local_light_ref.c"), os.path.join(DIR, "liblocallightref.so")
HOST_SRC, HOST_LIB = os.path.join(DIR, "local_light_host.cpp"), os.path.join(DIR, "liblocallighthost.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
# oracle/Makefile's CFLAGS: -ffp-contract=off is part of the definition
ORACLE_FLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-fopenmp", "-Wall", "-Wextra",
                "-Wno-unused-parameter", "-Wno-unused-function"]


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build():
    ref_deps = [REF_SRC] + [os.path.join(ORACLE, f) for f in ("or_light.c", "crychic_oracle.h", "or_math.h", "or_samplers.h", "or_gamma_pow.inc")]
    if _stale(REF_LIB, ref_deps):
        subprocess.run(["gcc"] + ORACLE_FLAGS + ["-I", ORACLE, "-shared", "-o", REF_LIB, REF_SRC, "-lm"], check=True)
    host_deps = [HOST_SRC, os.path.join(ROOT, "include", "crychic_hip.h")] + \
        [os.path.join(CSRC, f) for f in ("devmath.hpp", "gamma_pow.inc", "light_core.hpp")]
    if _stale(HOST_LIB, host_deps):
        subprocess.run([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, HOST_SRC, "-o", HOST_LIB], check=True)
    return REF_LIB, HOST_LIB


def _lights(lights):
    return (C.addressof(lights), len(lights)) if lights is not None and len(lights) else (None, 0)


class LocalLightLib:
    def __init__(self):
        ref, host = build()
        self._ref, self._host = C.CDLL(ref), C.CDLL(host)
        vp, u32, i, f = C.c_void_p, C.c_uint32, C.c_int, C.c_float
        args = [vp, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, vp, u32, u32, u32, u32, i, f, i, vp, u32, vp, u32, u32, u32, vp]
        self._ref.ss_deferred_light_spots_shadowed.argtypes = args
        self._host.shh_light_local.argtypes = args[:18] + [u32] + args[19:]     # flags: uint32_t there, int here
        for fn in (self._ref.ss_spot_shadow_factor, self._host.shh_spot_shadow_factor):
            fn.argtypes = [vp, u32, vp, vp]
            fn.restype = f

    def _run(self, fn, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots, maps, row0, rows, cube_dim):
        H, W = p["depth"].shape
        rows = H - row0 if rows is None else rows
        out = np.zeros((H, W, 4), np.uint8)
        rad = np.zeros((H, W, 4), np.float32)
        g = [np.ascontiguousarray(p[k], np.float32) for k in ("g0", "g1", "g2")]
        d = np.ascontiguousarray(p["depth"], np.uint32); s = np.ascontiguousarray(p["shadow"], np.uint32)
        c = np.ascontiguousarray(p["cube"], np.uint8)
        a = np.ascontiguousarray(ambient, np.uint16) if ambient is not None else None
        sh = (C.c_void_p * 4)(*[s[k].ctypes.data for k in range(4)])
        pp, pn = _lights(points)
        sp, sn = _lights(spots)
        m = None if maps is None or len(maps) == 0 else np.ascontiguousarray(maps, np.uint32)
        count, dim = (0, 0) if m is None else (m.shape[0], m.shape[1])
        mp = (C.c_void_p * 8)(*[m[k].ctypes.data for k in range(count)])
        fn(C.addressof(cb), g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, d.ctypes.data, a.ctypes.data if a is not None else None,
           sh, s.shape[1], c.ctypes.data, int(cube_dim or c.shape[1]), out.ctypes.data, rad.ctypes.data, W, H, row0, rows,
           num_dir_lights, pcf_radius, int(flags), pp, pn, sp, sn, count, dim, mp)
        return out, rad

    def checker(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, points=None, spots=None, maps=None, row0=0, rows=None,
                cube_dim=None):
        """The checker's frame (RGBA8, radiance).  cb: an oracle_lib.OrPassConstants (with the spot transforms in
        ShadowTransforms[4 + k] when there are maps); flags: the oracle's word (bit 0 sky, CRYCHIC_FIX_Q*, CRYCHIC_LIGHT_CUBE_LEVELS);
        points / spots: ctypes arrays of Light or None; maps: (count, dim, dim) uint32 D24 maps of the first `count` spot lights,
        or None for unshadowed spot lights."""
        return self._run(self._ref.ss_deferred_light_spots_shadowed, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots,
                         maps, row0, rows, cube_dim)

    def host(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, points=None, spots=None, maps=None, row0=0, rows=None,
             cube_dim=None):
        """The product's kernel body on the host (cb: the product's PassConstants; flags: the product's word): maps None models
        light_spots_kernel, maps given light_spots_shadowed_kernel."""
        return self._run(self._host.shh_light_local, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots,
                         maps, row0, rows, cube_dim)

    def factor(self, which, m, T, pos):
        """The shadow factor s of one position: which = "ref" (checker) or "host" (product body)."""
        m = np.ascontiguousarray(m, np.uint32)
        T = np.ascontiguousarray(T, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        fn = self._ref.ss_spot_shadow_factor if which == "ref" else self._host.shh_spot_shadow_factor
        return fn(m.ctypes.data, m.shape[0], T.ctypes.data, pos.ctypes.data)


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = LocalLightLib()
    return _LIB
