"""Builds and loads the spot-light test harness (TEST INFRASTRUCTURE ONLY): tests/spot_ref/libspotref.so, the checker (the frozen
oracle's or_light.c with the spot loop, built with the oracle's flags), and tests/spot_ref/libspothost.so, the product's spot-light
kernel body compiled for the host (as tests/hostsim does for the other bodies).  Both are rebuilt when a source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "spot_ref")
ORACLE = os.path.join(ROOT, "oracle")
CSRC = os.path.join(ROOT, "crychic_renderer_amd", "csrc")
REF_SRC, REF_LIB = os.path.join(DIR, "spot_ref.c"), os.path.join(DIR, "libspotref.so")
HOST_SRC, HOST_LIB = os.path.join(DIR, "spot_host.cpp"), os.path.join(DIR, "libspothost.so")
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


class SpotLib:
    def __init__(self):
        ref, host = build()
        self._ref, self._host = C.CDLL(ref), C.CDLL(host)
        vp, u32, i, f = C.c_void_p, C.c_uint32, C.c_int, C.c_float
        args = [vp, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, vp, u32, u32, u32, u32, i, f, i, vp, u32, vp, u32]
        self._ref.sr_deferred_light_spots.argtypes = args
        self._host.sh_light_spots.argtypes = args[:18] + [u32] + args[19:]        # flags: uint32_t there, int here

    def _run(self, fn, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots, row0, rows, cube_dim):
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
        fn(C.addressof(cb), g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, d.ctypes.data, a.ctypes.data if a is not None else None,
           sh, s.shape[1], c.ctypes.data, int(cube_dim or c.shape[1]), out.ctypes.data, rad.ctypes.data, W, H, row0, rows,
           num_dir_lights, pcf_radius, int(flags), pp, pn, sp, sn)
        return out, rad

    def checker(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, points=None, spots=None, row0=0, rows=None, cube_dim=None):
        """The checker's frame (RGBA8, radiance).  cb: an oracle_lib.OrPassConstants; flags: the oracle's word (bit 0 sky,
        CRYCHIC_FIX_Q*, CRYCHIC_LIGHT_CUBE_LEVELS); points / spots: ctypes arrays of Light or None."""
        return self._run(self._ref.sr_deferred_light_spots, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots, row0, rows, cube_dim)

    def host(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, points=None, spots=None, row0=0, rows=None, cube_dim=None):
        """The product's kernel body on the host (cb: the product's PassConstants; flags: the product's word)."""
        return self._run(self._host.sh_light_spots, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots, row0, rows, cube_dim)


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = SpotLib()
    return _LIB
