"""Frames and the host predicate for tests/test_ssao_prologue_gpu.py (TEST HARNESS ONLY): builds and loads
tests/hostsim/libssao_prologue_host.so -- the sky shortcut's predicate of csrc/ssao_core.hpp compiled for the host -- and makes the
sky-over-geometry frames whose wavefronts it classifies."""
import ctypes as C
import os

import numpy as np

import hostsim_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "ssao_prologue_host.cpp")
LIB = os.path.join(ROOT, "tests", "hostsim", "libssao_prologue_host.so")


def build():
    return hostsim_lib.build_host(LIB, SRC, ("ssao_core.hpp",))


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.sp_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _LIB.sp_cell_of_lane_mismatches.restype = C.c_uint32
    return _LIB


FIELDS = ("taken", "refused", "lit", "max_cells", "fallback", "over_64", "sky_enabled", "cull_enabled", "lane_mismatches")


def classify(cb, normal, depth, row0=0, rows=None):
    """The wavefronts of an SSAO pass over half-res rows [row0, row0 + rows), as ssao_kernel sorts them (ssao_prologue_host.cpp)."""
    H, W = depth.shape
    rows = H // 2 - row0 if rows is None else rows
    out = np.zeros(9, np.uint32)
    n = np.ascontiguousarray(normal.view(np.uint16)); d = np.ascontiguousarray(depth)
    load().sp_classify(C.addressof(cb), n.ctypes.data, d.ctypes.data, W, H, row0, rows, out.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in out)))


def constants(W, H, sky=True, cull=True, radius=None):
    """SSAO constants with the sky shortcut and the tap culling each on or off, switched the way a caller switches them -- through
    the constants the host guards look at (ssao_sky_reach, ssao_cull_params):
      sky off:  SurfaceEpsilon 0.001, below 2^-16 of the far distance 100 (the shortcut's and the clear cells' guard);
      cull off: near plane 1e-4, so that Proj[2][2] = far / (far - near) is not above 1.000002 (the culling's guard).
    radius: OcclusionRadius (the sky reach grows with it)."""
    from crychic_renderer_amd import scene
    cam = scene.default_camera(W, H)
    if not cull:
        cam.nearZ = 1.0e-4
    c = scene.Constants(W, H, shadow_dim=64, cam=cam)
    if not sky:
        c.ssao_cb.SurfaceEpsilon = 0.001
    if radius is not None:
        c.ssao_cb.OcclusionRadius = radius
    return c


def sky_over_geometry(cb, W, H, seed, horizon=None):
    """Sky (clear depth, normal (0, 0, -1)) over rough ground: the horizon, tilted by a few rows across the frame, at texel row
    `horizon` (default: just past the middle, on an odd row, so that half-res pixels straddle it).  Ground view depth falls from
    60 % of the far distance at the horizon to a few units at the bottom, with bumps that occlude.  horizon >= H: all sky."""
    rng = np.random.default_rng(4200 + seed)
    A, B = cb.Proj[10], cb.Proj[11]
    far = B / (1.0 - A)
    horizon = (H // 2 + 6) | 1 if horizon is None else horizon
    depth = np.full((H, W), 0xFFFFFF, dtype=np.uint32)
    normal = np.zeros((H, W, 4), dtype=np.float16); normal[..., 2] = -1.0
    yy, xx = np.mgrid[0:H, 0:W]
    hz = horizon + (xx * 5) // W                                     # tilted: 0 .. 4 rows lower on the right
    t = np.clip((yy - hz) / max(1.0, float(H - horizon)), 0.0, 1.0)
    vz = 0.6 * far * (1.0 - t) + 3.0 * t + rng.uniform(0.0, 0.8, size=(H, W))
    d = np.clip(np.round((A + B / vz) * 16777215.0), 0, 0xFFFFFE).astype(np.uint32)
    ground = yy >= hz
    depth[ground] = d[ground]
    nn = rng.standard_normal((H, W, 3)).astype(np.float16) * np.float16(0.4); nn[..., 2] -= np.float16(1.0)
    normal[ground, :3] = nn[ground]
    randvec = rng.integers(0, 256, size=(256, 256, 4), dtype=np.uint8)
    return depth, normal, randvec

