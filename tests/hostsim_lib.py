"""Builds and loads tests/hostsim/libhostsim.so: the product's per-pixel kernel bodies compiled for the host
(TEST HARNESS ONLY -- lets the CPU-only tier compare the kernel text with the oracle bit for bit)."""
import ctypes as C
import os
import subprocess

import numpy as np

from gbuffer_f16_lib import F16_MASK, G0_F16, G1_F16, G2_F16
from oracle_lib import draw_item_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim.cpp")
LIB = os.path.join(ROOT, "tests", "hostsim", "libhostsim.so")
CSRC = os.path.join(ROOT, "crychic_renderer_amd", "csrc")
HOST_LIGHT = os.path.join(ROOT, "tests", "hostsim", "host_light.hpp")      # the lighting call every host harness shares
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


SANITIZE = os.environ.get("CRYCHIC_SANITIZE") == "1"      # tools/sanitize.sh: ASan + UBSan build of the kernel bodies
SAN_DIR = os.path.join(ROOT, "tests", "hostsim", "_san")
SAN_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-shared-libsan"]


def build_sanitized(name, sources, extra=()):
    """clang ASan + UBSan shared object under tests/hostsim/_san (loaded with the sanitizer runtime preloaded: tools/sanitize.sh)."""
    os.makedirs(SAN_DIR, exist_ok=True)
    out = os.path.join(SAN_DIR, name)
    deps = list(sources) + [HOST_LIGHT] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "crychic_hip.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run([CLANG, "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma"] + SAN_FLAGS + list(extra) +
                       ["-I", os.path.join(ROOT, "include"), "-I", CSRC] + list(sources) + ["-o", out], check=True)
    return out


def build_host(lib, src, headers):
    """The host harness `lib` from its one source `src`, rebuilt when the source, host_light.hpp or one of csrc's `headers` (besides
    the ones every harness includes) is newer; with CRYCHIC_SANITIZE=1 its ASan + UBSan build instead."""
    if SANITIZE:
        return build_sanitized(os.path.basename(lib), [src])
    deps = [src, HOST_LIGHT] + [os.path.join(CSRC, f) for f in ("devmath.hpp", "gamma_pow.inc", "light_core.hpp", "light_bind.hpp") + tuple(headers)]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.run([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, src, "-o", lib], check=True)
    return lib


DEVMATH_EVAL = os.path.join(ROOT, "tests", "hostsim", "devmath_eval.hpp")      # hs_eval_array's kinds (shared with tests/devmath_dev)


def build():
    # a dependency build_host does not know: a library older than it is built again
    for lib in (LIB, os.path.join(SAN_DIR, os.path.basename(LIB))):
        if os.path.exists(lib) and os.path.getmtime(DEVMATH_EVAL) > os.path.getmtime(lib):
            os.remove(lib)
    return build_host(LIB, SRC, ("ssao_core.hpp", "blur_tiles.hpp", "raster_core.hpp"))


G_F16 = (G0_F16, G1_F16, G2_F16)


def _lights(lights):
    return (C.addressof(lights), len(lights)) if lights is not None and len(lights) else (None, 0)


# hs_light's arguments; the checkers' entry points (ss_deferred_light_spots_shadowed: the first 26, ps_deferred_light_point_shadows:
# all 30) take the same leading ones, with flags as an int
LIGHT_ARGTYPES = [C.c_void_p] * 7 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + \
    [C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]


def run_light(fn, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, points=None, spots=None, maps=None, cubes=None, projs=None,
              row0=0, rows=None, cube_dim=None, formats=False):
    """One lighting call through fn, an entry point with (a prefix of) hs_light's arguments: the product's body on the host or a
    checker.  p: the planes (g0..g2, depth, shadow, cube); points / spots: ctypes arrays of Light or None; maps: (count, dim, dim)
    uint32 D24 maps of the first `count` spot lights; cubes: (count, 6, dim, dim) uint32 D24 faces of the first `count` point
    lights, and projs, their (count, 16) untransposed shadow projections.  formats: G-buffer planes may be float16 arrays, and
    their formats go into the flags word (the CRYCHIC_GBUFFER_G*_F16 bits); otherwise the planes are taken as float32.
    Returns (RGBA8, radiance)."""
    H, W = p["depth"].shape
    rows = H - row0 if rows is None else rows
    out = np.zeros((H, W, 4), np.uint8)
    rad = np.zeros((H, W, 4), np.float32)
    g = [np.ascontiguousarray(p[k], None if formats else np.float32) for k in ("g0", "g1", "g2")]
    assert all(x.dtype in (np.float32, np.float16) for x in g)
    flags = int(flags)
    if formats:
        flags = (flags & ~F16_MASK) | sum(bit for x, bit in zip(g, G_F16) if x.dtype == np.float16)
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
    args = (C.addressof(cb), g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, d.ctypes.data, a.ctypes.data if a is not None else None,
            sh, s.shape[1], c.ctypes.data, int(cube_dim or c.shape[1]), out.ctypes.data, rad.ctypes.data, W, H, row0, rows,
            num_dir_lights, pcf_radius, flags, pp, pn, sp, sn, count, dim, mp, pcount, pdim, qp, T.ctypes.data)
    assert pcount == 0 or len(fn.argtypes) == len(args), "this entry point takes no point shadows"
    fn(*args[:len(fn.argtypes)])
    return out, rad


class HostSim:
    def __init__(self):
        self.lib = L = C.CDLL(build())
        f, u32, i, vp = C.c_float, C.c_uint32, C.c_int, C.c_void_p
        for n in ("hs_d24_to_float", "hs_unorm16_to_float", "hs_unorm8_to_float"):
            getattr(L, n).restype = f; getattr(L, n).argtypes = [u32]
        L.hs_half_to_float.restype = f; L.hs_half_to_float.argtypes = [C.c_uint16]
        L.hs_float_to_half.restype = C.c_uint16; L.hs_float_to_half.argtypes = [f]
        for n in ("hs_det_sin", "hs_det_cos", "hs_det_log2", "hs_det_exp2"):
            getattr(L, n).restype = f; getattr(L, n).argtypes = [f]
        L.hs_det_pow.restype = f; L.hs_det_pow.argtypes = [f, f]
        L.hs_nrand.restype = f; L.hs_nrand.argtypes = [f, f]
        L.hs_check_d24_threshold.restype = u32
        L.hs_eval_array.argtypes = [i, C.c_size_t, vp, vp, vp]
        L.hs_ssao.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, u32, u32]
        L.hs_ssao_path.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, i]
        L.hs_ssao_guards.argtypes = [vp, u32, u32, vp]
        L.hs_last_sky_waves.restype = u32
        L.hs_last_culled_taps.restype = u32
        L.hs_last_clear_cell_taps.restype = u32
        L.hs_blur.argtypes = [vp, vp, vp, vp, u32, u32, i, u32, u32]
        L.hs_blur_chain.argtypes = [vp, vp, vp, vp, u32, u32, i, u32, u32, i, i]
        L.hs_last_settled_tiles.restype = u32
        L.hs_blur_chain_ssao_plane.restype = i; L.hs_blur_chain_ssao_plane.argtypes = [i]
        L.hs_blur_chain_ssao_rows.argtypes = [i, u32, u32, u32, vp, vp]
        L.hs_set_stamp.argtypes = [u32]
        L.hs_set_prep_margin.argtypes = [i]
        L.hs_last_unprepared_rows.restype = u32
        L.hs_rasterize.restype = i
        L.hs_rasterize.argtypes = [i, vp, vp, vp, u32, vp, u32, vp, u32, u32, u32, i, f, vp, vp, vp, vp, vp, u32, u32, u32]
        L.hs_light.argtypes = LIGHT_ARGTYPES
        L.hs_light_tiled.argtypes = LIGHT_ARGTYPES + [vp]
        L.hs_spot_shadow_factor.restype = f; L.hs_spot_shadow_factor.argtypes = [vp, u32, vp, vp]
        L.hs_point_shadow_factor.restype = f; L.hs_point_shadow_factor.argtypes = [vp, u32, vp, vp, vp]
        L.hs_point_face.restype = i; L.hs_point_face.argtypes = [vp, vp]

    def eval_array(self, kind, a, b=None):
        a = np.ascontiguousarray(a); out = np.zeros(a.shape, dtype=np.float32)
        b = np.ascontiguousarray(b) if b is not None else a
        self.lib.hs_eval_array(kind, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data)
        return out

    def ssao(self, cb, normal_f16, depth_u32, randvec_u8, edge_bytes, row0=0, rows=None, emit=True, pairs=True, cull=True, edge=None, stamp=1, margin=-1):
        """pairs=True: the taps gather from the decoded depth-pairs plane (the product's path when it has a workspace), and with
        cull=True skip the ones the nearest-depth map proves to add nothing; pairs=False: from the raw D24 plane.
        edge: a workspace to (re)use as it is -- like the device, nothing clears it; stamp: the frame stamp of this call;
        margin: texel rows the depth pass visits beyond the rows of the call (-1: the product's default)."""
        H, W = depth_u32.shape
        rows = H // 2 - row0 if rows is None else rows
        out = np.zeros((H // 2, W // 2), dtype=np.uint16)
        if edge is None:
            edge = np.zeros((edge_bytes,), dtype=np.uint8)
        n = np.ascontiguousarray(normal_f16.view(np.uint16)); d = np.ascontiguousarray(depth_u32); r = np.ascontiguousarray(randvec_u8)
        self.lib.hs_set_stamp(int(stamp))
        self.lib.hs_set_prep_margin(int(margin))
        self.lib.hs_ssao_path(C.addressof(cb), n.ctypes.data, d.ctypes.data, r.ctypes.data, out.ctypes.data if emit else None,
                              edge.ctypes.data, W, H, row0, rows, (1 if cull else 2) if pairs else 0)
        return out, edge

    def ssao_guards(self, cb, W, H):
        """What the launchers' guards decide for cb on a W x H frame, from the product's own functions: a dict of sparse, sky, rx,
        ry, cull, clear, weights (hs_ssao_guards)."""
        out = (C.c_uint32 * 7)()
        self.lib.hs_ssao_guards(C.addressof(cb), W, H, out)
        return dict(zip(("sparse", "sky", "rx", "ry", "cull", "clear", "weights"), (int(v) for v in out)))

    def blur(self, cb, edge, ambient_in, W, H, horizontal, row0=0, rows=None):
        rows = H // 2 - row0 if rows is None else rows
        out = np.zeros((H // 2, W // 2), dtype=np.uint16)
        a = np.ascontiguousarray(ambient_in)
        self.lib.hs_blur(C.addressof(cb), edge.ctypes.data, a.ctypes.data, out.ctypes.data, W, H, 1 if horizontal else 0, row0, rows)
        return out

    def compute_ssao(self, cb, normal_f16, depth_u32, randvec_u8, edge_bytes, blur_count, row0=0, rows=None, use_exit=True, ones_margin=None,
                     edge=None, stamp=1, margin=-1):
        """Ssao::ComputeSsao the way api.cpp sequences it (SSAO pass, then the two-launch blur chain of blur_tiles.hpp through the
        kernels' own tile bodies).  Returns (ambient0, edge); rows [row0, row0 + rows) of ambient0 are the result.
        ones_margin: the reach the unoccluded-tile exit assumes (default: what api.cpp passes, 5 per iteration)."""
        H, W = depth_u32.shape
        h2 = H // 2
        rows = h2 - row0 if rows is None else rows
        r0, rn = C.c_uint32(), C.c_uint32()
        self.lib.hs_blur_chain_ssao_rows(blur_count, row0, rows, h2, C.addressof(r0), C.addressof(rn))
        out, edge = self.ssao(cb, normal_f16, depth_u32, randvec_u8, edge_bytes, r0.value, rn.value, edge=edge, stamp=stamp, margin=margin)
        planes = [np.full((h2, W // 2), 0xABCD, dtype=np.uint16), np.full((h2, W // 2), 0xABCD, dtype=np.uint16)]     # junk where nothing writes
        sp = self.lib.hs_blur_chain_ssao_plane(blur_count)
        planes[sp][r0.value:r0.value + rn.value] = out[r0.value:r0.value + rn.value]
        self.lib.hs_blur_chain(C.addressof(cb), edge.ctypes.data, planes[0].ctypes.data, planes[1].ctypes.data, W, H, blur_count, row0, rows,
                               1 if use_exit else 0, 5 * blur_count if ones_margin is None else int(ones_margin))
        return planes[0], edge

    def blur_chain(self, cb, edge, ambient_in, W, H, blur_count, use_exit=False):
        """The blur chain alone on a caller-made ambient map (whole frame, no exit unless the workspace's map belongs to it)."""
        h2 = H // 2
        planes = [np.full((h2, W // 2), 0xABCD, dtype=np.uint16), np.full((h2, W // 2), 0xABCD, dtype=np.uint16)]
        planes[self.lib.hs_blur_chain_ssao_plane(blur_count)][:] = ambient_in
        self.lib.hs_blur_chain(C.addressof(cb), edge.ctypes.data, planes[0].ctypes.data, planes[1].ctypes.data, W, H, blur_count, 0, h2,
                               1 if use_exit else 0, 5 * blur_count)
        return planes[0]

    def rasterize(self, mode, view_t, viewproj_t, items, materials, textures, W, H, depth_bias=0, slope_bias=0.0, *, mix=0,
                  g_row0=0, g_rows=0, fill=0):
        """The producer passes on the host.  mode 0: depth (the shadow pass, biased); 1: depth + normals; 2: the G-buffer pass;
        3: the fused pass (crychic_draw_gbuffer_formats with normals).  mix: the CRYCHIC_GBUFFER_G*_F16 bits of G0..G2;
        g_row0 / g_rows: the rows G0..G2 are written for (g_rows 0: the whole target).  Every output starts filled with the byte
        `fill`, so texels the pass leaves untouched show.  Returns depth, normal (or None) and g0..g2 (or None)."""
        from crychic_renderer_amd._lib import DrawItem, Texture
        from crychic_renderer_amd.geometry import texture_levels
        arr = (DrawItem * len(items))()
        keep = []
        for k, item in enumerate(items):                     # 3-tuples, or 5-tuples with the two locations (oracle_lib.draw_item_fields)
            arr[k] = DrawItem(*draw_item_fields(item, keep))
        tex = (Texture * max(1, len(textures or [])))()
        for k, t in enumerate(textures or []):
            if t is not None:
                flat, tw, th, levels = texture_levels(t); keep.append(flat)
                tex[k] = Texture(flat.ctypes.data, tw, th, levels)
        mats = np.ascontiguousarray(materials) if materials is not None else None
        byte = np.uint8(fill)
        depth = np.full((H, W, 4), byte, np.uint8).view(np.uint32).reshape(H, W)
        normal = np.full((H, W, 8), byte, np.uint8).view(np.uint16) if mode & 1 else None
        g = [np.full((H, W, 8 if mix & bit else 16), byte, np.uint8).view(np.float16 if mix & bit else np.float32) if mode & 2 else None
             for bit in G_F16]
        view_t = np.ascontiguousarray(view_t, np.float32); viewproj_t = np.ascontiguousarray(viewproj_t, np.float32)
        n = self.lib.hs_rasterize(mode, view_t.ctypes.data, viewproj_t.ctypes.data, arr, len(items),
                                  mats.ctypes.data if mats is not None else None, len(mats) if mats is not None else 0,
                                  tex if textures else None, len(textures or []), W, H, depth_bias, slope_bias, depth.ctypes.data,
                                  normal.ctypes.data if normal is not None else None, *[x.ctypes.data if x is not None else None for x in g],
                                  mix, g_row0, g_rows)
        if n < 0:
            raise RuntimeError("hs_rasterize failed (%d)" % n)
        return {"depth": depth, "normal": normal.view(np.float16) if normal is not None else None, "g0": g[0], "g1": g[1], "g2": g[2], "tris": n}

    def float_to_half(self, x):
        """raster_core.hpp float_to_half of every element of x (float32) -> uint16 bits."""
        x = np.ascontiguousarray(x, np.float32)
        return np.array([self.lib.hs_float_to_half(float(v)) for v in x.reshape(-1)], np.uint16).reshape(x.shape)

    def half_to_float(self, h):
        h = np.ascontiguousarray(h, np.uint16)
        return np.array([self.lib.hs_half_to_float(int(v)) for v in h.reshape(-1)], np.float32).reshape(h.shape)

    def light_frame(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, **lights):
        """One lighting call of the product's body on the host over the planes p (cb: the product's PassConstants; flags: the
        product's word -- sky, CRYCHIC_FIX_Q*, CRYCHIC_LIGHT_CUBE_LEVELS; the plane formats come from the dtypes of g0..g2).
        lights: points, spots, maps, cubes, projs, row0, rows, cube_dim as run_light takes them; which kernel family that models
        is light_bind.hpp's choice, as in the library.  Returns (RGBA8, radiance)."""
        return run_light(self.lib.hs_light, cb, p, ambient, num_dir_lights, pcf_radius, flags, formats=True, **lights)

    def light_frame_tiled(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, **lights):
        """light_frame with the local lights culled per 64 x 4 tile as the kernels cull them (host_light.hpp's tiled mode: tiles
        anchored at row0, box and admitted lights from light_core.hpp's tile_box_* / tile_light_touches).  Returns (RGBA8, radiance,
        masks): masks[ty, tx, 0] are the 32 words of tile (tx, ty)'s point-light mask and masks[ty, tx, 1] the spot lights', bit
        l & 31 of word l >> 5 set = light l admitted; ty counts from row0."""
        H, W = p["depth"].shape
        row0 = lights.get("row0", 0)
        rows = H - row0 if lights.get("rows") is None else lights["rows"]
        masks = np.zeros(((rows + 3) // 4, (W + 63) // 64, 2, 32), np.uint32)

        def fn(*args):
            self.lib.hs_light_tiled(*args, masks.ctypes.data)
        fn.argtypes = LIGHT_ARGTYPES
        out, rad = run_light(fn, cb, p, ambient, num_dir_lights, pcf_radius, flags, formats=True, **lights)
        return out, rad, masks

    def light(self, cb, g0, g1, g2, depth_u32, ambient, shadow_u32, cube_u8, num_dir_lights, pcf_radius, flags=0,
              want_radiance=False, point_lights=None, cube_dim=None, cube_levels=0, **lights):
        """light_frame over separate planes, with the chain's level count as an argument; RGBA8 alone unless want_radiance."""
        p = {"g0": g0, "g1": g1, "g2": g2, "depth": depth_u32, "shadow": shadow_u32, "cube": cube_u8}
        out, rad = self.light_frame(cb, p, ambient, num_dir_lights, pcf_radius, int(flags) | ((int(cube_levels) & 15) << 16),
                                    points=point_lights, cube_dim=cube_dim, **lights)
        return (out, rad) if want_radiance else out

    def spot_shadow_factor(self, m, T, pos):
        """spot_shadow_factor of one position in the (dim, dim) D24 map m under the transposed transform T."""
        m = np.ascontiguousarray(m, np.uint32)
        T = np.ascontiguousarray(T, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        return self.lib.hs_spot_shadow_factor(m.ctypes.data, m.shape[0], T.ctypes.data, pos.ctypes.data)

    def point_shadow_factor(self, faces, proj, light_pos, pos):
        """PointShadowOf of one position: faces (6, dim, dim), proj the light's untransposed shadow projection."""
        faces = np.ascontiguousarray(faces, np.uint32)
        proj = np.ascontiguousarray(proj, np.float32).reshape(16)
        lp = np.ascontiguousarray(light_pos, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        return self.lib.hs_point_shadow_factor(faces.ctypes.data, faces.shape[1], proj.ctypes.data, lp.ctypes.data, pos.ctypes.data)

    def point_face(self, v):
        """(f, (a, b, c)) of point_face."""
        v = np.ascontiguousarray(v, np.float32)
        abc = np.zeros(3, np.float32)
        return self.lib.hs_point_face(v.ctypes.data, abc.ctypes.data), abc


_HS = None


def load():
    global _HS
    if _HS is None:
        _HS = HostSim()
    return _HS
