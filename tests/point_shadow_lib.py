"""Builds and loads the shadowed point-light test harness (TEST INFRASTRUCTURE ONLY): tests/point_shadow_ref/libpointshadowref.so,
the checker (tests/local_light_ref/local_light_ref.c included unchanged, with the cube face step and a shadowed point term, built with
the oracle's flags), and tests/point_shadow_ref/libpointshadowhost.so, the product's kernel body compiled for the host.  Both are
rebuilt when a source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

import local_light_lib
from local_light_lib import CLANG, CSRC, ORACLE, ORACLE_FLAGS, ROOT, _lights, _stale

DIR = os.path.join(ROOT, "tests", "point_shadow_ref")
REF_SRC, REF_LIB = os.path.join(DIR, "point_shadow_ref.c"), os.path.join(DIR, "libpointshadowref.so")
HOST_SRC, HOST_LIB = os.path.join(DIR, "point_shadow_host.cpp"), os.path.join(DIR, "libpointshadowhost.so")


def build():
    ref_deps = [REF_SRC, local_light_lib.REF_SRC] + \
        [os.path.join(ORACLE, f) for f in ("or_light.c", "crychic_oracle.h", "or_math.h", "or_samplers.h", "or_gamma_pow.inc")]
    if _stale(REF_LIB, ref_deps):
        subprocess.run(["gcc"] + ORACLE_FLAGS + ["-I", ORACLE, "-shared", "-o", REF_LIB, REF_SRC, "-lm"], check=True)
    host_deps = [HOST_SRC, os.path.join(ROOT, "include", "crychic_hip.h")] + \
        [os.path.join(CSRC, f) for f in ("devmath.hpp", "gamma_pow.inc", "light_core.hpp")]
    if _stale(HOST_LIB, host_deps):
        subprocess.run([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, HOST_SRC, "-o", HOST_LIB], check=True)
    return REF_LIB, HOST_LIB


class PointShadowLib:
    def __init__(self):
        ref, host = build()
        self._ref, self._host = C.CDLL(ref), C.CDLL(host)
        vp, u32, i, f = C.c_void_p, C.c_uint32, C.c_int, C.c_float
        args = [vp, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, vp, u32, u32, u32, u32, i, f, i, vp, u32, vp, u32, u32, u32, vp,
                u32, u32, vp, vp]
        self._ref.ps_deferred_light_point_shadows.argtypes = args
        self._host.psh_light_point_shadows.argtypes = args[:18] + [u32] + args[19:]     # flags: uint32_t there, int here
        for fn in (self._ref.ps_point_shadow_factor, self._host.psh_point_shadow_factor):
            fn.argtypes = [vp, u32, vp, vp, vp]
            fn.restype = f
        for fn in (self._ref.ps_point_face, self._host.psh_point_face):
            fn.argtypes = [vp, vp]
            fn.restype = i

    def _run(self, fn, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots, maps, cubes, projs, row0, rows, cube_dim):
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
        q = None if cubes is None or len(cubes) == 0 else np.ascontiguousarray(cubes, np.uint32)
        pcount, pdim = (0, 0) if q is None else (q.shape[0], q.shape[2])
        qp = (C.c_void_p * 4)(*[q[k].ctypes.data for k in range(pcount)])
        T = np.ascontiguousarray(np.zeros((4, 16), np.float32) if projs is None else np.asarray(projs, np.float32).reshape(-1, 16))
        fn(C.addressof(cb), g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, d.ctypes.data, a.ctypes.data if a is not None else None,
           sh, s.shape[1], c.ctypes.data, int(cube_dim or c.shape[1]), out.ctypes.data, rad.ctypes.data, W, H, row0, rows,
           num_dir_lights, pcf_radius, int(flags), pp, pn, sp, sn, count, dim, mp, pcount, pdim, qp, T.ctypes.data)
        return out, rad

    def checker(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, points=None, spots=None, maps=None, cubes=None, projs=None,
                row0=0, rows=None, cube_dim=None):
        """The checker's frame (RGBA8, radiance): local_light_lib's checker plus cubes, (count, 6, dim, dim) uint32 D24 faces of the
        first `count` point lights, and projs, their (count, 16) untransposed shadow projections.  cubes None: no point shadows."""
        return self._run(self._ref.ps_deferred_light_point_shadows, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots,
                         maps, cubes, projs, row0, rows, cube_dim)

    def host(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, points=None, spots=None, maps=None, cubes=None, projs=None,
             row0=0, rows=None, cube_dim=None):
        """The product's kernel body on the host (cb: the product's PassConstants; flags: the product's word)."""
        return self._run(self._host.psh_light_point_shadows, cb, p, ambient, num_dir_lights, pcf_radius, flags, points, spots,
                         maps, cubes, projs, row0, rows, cube_dim)

    def factor(self, which, faces, proj, light_pos, pos):
        """The cube shadow factor s of one position: which = "ref" (checker) or "host" (product body); faces (6, dim, dim)."""
        faces = np.ascontiguousarray(faces, np.uint32)
        proj = np.ascontiguousarray(proj, np.float32).reshape(16)
        lp = np.ascontiguousarray(light_pos, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        fn = self._ref.ps_point_shadow_factor if which == "ref" else self._host.psh_point_shadow_factor
        return fn(faces.ctypes.data, faces.shape[1], proj.ctypes.data, lp.ctypes.data, pos.ctypes.data)

    def face(self, which, v):
        """(f, (a, b, c)) of the face step: which = "ref" or "host"."""
        v = np.ascontiguousarray(v, np.float32)
        abc = np.zeros(3, np.float32)
        fn = self._ref.ps_point_face if which == "ref" else self._host.psh_point_face
        f = fn(v.ctypes.data, abc.ctypes.data)
        return f, abc


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = PointShadowLib()
    return _LIB
