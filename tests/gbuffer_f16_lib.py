"""Builds and loads the G-buffer format test harness (TEST INFRASTRUCTURE ONLY): tests/gbuffer_f16_ref/libgbufferf16host.so, the
product's format-aware load path + light_pixel and its format-aware resolve compiled for the host (as tests/hostsim and
tests/point_shadow_ref do for the other bodies).  Rebuilt when a source is newer.  There is no checker library of its own: the
contract is stated against the frozen checkers on the WIDENED planes (oracle_lib, local_light_lib, point_shadow_lib) and against
numpy.float16 of the oracle rasteriser's fp32 planes."""
import ctypes as C
import os
import subprocess

import numpy as np

from local_light_lib import CLANG, CSRC, ROOT, _lights, _stale

DIR = os.path.join(ROOT, "tests", "gbuffer_f16_ref")
HOST_SRC, HOST_LIB = os.path.join(DIR, "gbuffer_f16_host.cpp"), os.path.join(DIR, "libgbufferf16host.so")

G0_F16, G1_F16, G2_F16 = 0x1000, 0x2000, 0x4000          # CRYCHIC_GBUFFER_G*_F16
F16_MASK = 0x7000
MIXES = [m << 12 for m in range(8)]                      # all eight format mixes, as flag bits
MIXED, ALL_F16 = G1_F16 | G2_F16, F16_MASK               # "mixed": G0 float4, G1 + G2 half4; "f16": all three half4


def build():
    deps = [HOST_SRC, os.path.join(ROOT, "include", "crychic_hip.h")] + \
        [os.path.join(CSRC, f) for f in ("devmath.hpp", "gamma_pow.inc", "light_core.hpp", "raster_core.hpp")]
    if _stale(HOST_LIB, deps):
        subprocess.run([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, HOST_SRC, "-o", HOST_LIB], check=True)
    return HOST_LIB


def pack_planes(p, mix):
    """The planes of p with G0..G2 stored in the formats of `mix`: a half plane is numpy's float32 -> float16 conversion (round to
    nearest even, subnormals kept, overflow to infinity -- tests/test_gbuffer_f16_host.py holds it against float_to_half)."""
    q = dict(p)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(3):
            g = np.ascontiguousarray(p["g%d" % k], np.float32)
            q["g%d" % k] = g.astype(np.float16) if mix & (G0_F16 << k) else g
    return q


def widen_planes(p):
    """The planes of p with every G-buffer plane as float32 (a half plane widens exactly): what the frozen checkers are run on."""
    q = dict(p)
    for k in range(3):
        q["g%d" % k] = np.ascontiguousarray(p["g%d" % k]).astype(np.float32)
    return q


def mix_of(p):
    """The CRYCHIC_GBUFFER_* bits of the planes' dtypes."""
    return sum((G0_F16 << k) for k in range(3) if p["g%d" % k].dtype == np.float16)


class GBufferF16Lib:
    def __init__(self):
        self._host = C.CDLL(build())
        vp, u32, i, f = C.c_void_p, C.c_uint32, C.c_int, C.c_float
        self._host.gfh_light.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, vp, u32, u32, u32, u32, i, f, u32, vp, u32, vp, u32,
                                         u32, u32, vp, u32, u32, vp, vp]
        self._host.gfh_float_to_half.argtypes = [f]; self._host.gfh_float_to_half.restype = C.c_uint16
        self._host.gfh_half_to_float.argtypes = [C.c_uint16]; self._host.gfh_half_to_float.restype = f
        self._host.gfh_rasterize.restype = i
        self._host.gfh_rasterize.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32]

    def float_to_half(self, x):
        """raster_core.hpp float_to_half of every element of x (float32) -> uint16 bits."""
        x = np.ascontiguousarray(x, np.float32)
        return np.array([self._host.gfh_float_to_half(float(v)) for v in x.reshape(-1)], np.uint16).reshape(x.shape)

    def half_to_float(self, h):
        h = np.ascontiguousarray(h, np.uint16)
        return np.array([self._host.gfh_half_to_float(int(v)) for v in h.reshape(-1)], np.float32).reshape(h.shape)

    def light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, points=None, spots=None, maps=None, cubes=None, projs=None,
              row0=0, rows=None, cube_dim=None):
        """The product's format-aware body on the host: p's G-buffer planes are float32 or float16 arrays, and their formats go into
        the flags word beside `flags` (the product's word: sky, CRYCHIC_FIX_Q*, CRYCHIC_LIGHT_CUBE_LEVELS).  Lights, maps, cubes and
        projs as point_shadow_lib.  Returns (RGBA8, radiance)."""
        H, W = p["depth"].shape
        rows = H - row0 if rows is None else rows
        out = np.zeros((H, W, 4), np.uint8)
        rad = np.zeros((H, W, 4), np.float32)
        g = [np.ascontiguousarray(p[k]) for k in ("g0", "g1", "g2")]
        assert all(x.dtype in (np.float32, np.float16) for x in g)
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
        self._host.gfh_light(C.addressof(cb), g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, d.ctypes.data,
                             a.ctypes.data if a is not None else None, sh, s.shape[1], c.ctypes.data, int(cube_dim or c.shape[1]),
                             out.ctypes.data, rad.ctypes.data, W, H, row0, rows, num_dir_lights, pcf_radius,
                             (int(flags) & ~F16_MASK) | mix_of(p), pp, pn, sp, sn, count, dim, mp, pcount, pdim, qp, T.ctypes.data)
        return out, rad

    def rasterize(self, view_t, viewproj_t, items, materials, textures, W, H, mix, with_normals=False, g_row0=0, g_rows=0, fill=0xCD):
        """crychic_draw_gbuffer_formats on the host (the fused pass when with_normals).  Every output starts filled with the byte
        `fill`, so texels the pass leaves untouched show.  Returns depth, normal (or None) and g0..g2 in the formats of `mix`."""
        from crychic_renderer_amd._lib import DrawItem, Texture
        from crychic_renderer_amd.geometry import texture_levels
        arr = (DrawItem * len(items))()
        keep = []
        for k, (v, idx, inst) in enumerate(items):
            v = np.ascontiguousarray(v); idx = np.ascontiguousarray(idx); inst = np.ascontiguousarray(inst)
            keep += [v, idx, inst]
            arr[k] = DrawItem(v.ctypes.data, len(v), idx.ctypes.data, len(idx), 0, 0, inst.ctypes.data, len(inst))
        tex = (Texture * max(1, len(textures or [])))()
        for k, t in enumerate(textures or []):
            if t is not None:
                flat, tw, th, levels = texture_levels(t); keep.append(flat)
                tex[k] = Texture(flat.ctypes.data, tw, th, levels)
        mats = np.ascontiguousarray(materials) if materials is not None else None
        byte = np.uint8(fill)
        depth = np.full((H, W), byte, np.uint8).repeat(4, axis=1).view(np.uint32)
        normal = np.full((H, W, 8), byte, np.uint8).view(np.uint16) if with_normals else None
        g = [np.full((H, W, 8 if mix & (G0_F16 << k) else 16), byte, np.uint8).view(np.float16 if mix & (G0_F16 << k) else np.float32)
             for k in range(3)]
        view_t = np.ascontiguousarray(view_t, np.float32); viewproj_t = np.ascontiguousarray(viewproj_t, np.float32)
        n = self._host.gfh_rasterize(view_t.ctypes.data, viewproj_t.ctypes.data, arr, len(items),
                                     mats.ctypes.data if mats is not None else None, len(mats) if mats is not None else 0,
                                     tex if textures else None, len(textures or []), W, H, depth.ctypes.data,
                                     normal.ctypes.data if normal is not None else None, g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data,
                                     mix, g_row0, g_rows)
        if n < 0:
            raise RuntimeError("gfh_rasterize failed (%d)" % n)
        return {"depth": depth, "normal": normal.view(np.float16) if normal is not None else None, "g0": g[0], "g1": g[1], "g2": g[2], "tris": n}


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = GBufferF16Lib()
    return _LIB
