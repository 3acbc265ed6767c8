"""Builds and loads tests/ssr_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_ssr, plain C written from the definition in
include/crychic_hip.h with none of the kernel's code; the corpus of frames, images and parameter sets the host and the device tests
share; and the mirror scene of the definition's anchor, built by float64 ray casting."""
import ctypes as C
import math
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share
import fog_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "ssr_ref")
SRC, LIB = os.path.join(DIR, "ssr_ref.c"), os.path.join(DIR, "libssrref.so")
GOLD = os.path.join(ROOT, "tests", "golden", "frame_64x64.npz")

COUNTERS = ("sky", "rough", "behind_near", "near_clipped", "own_skip", "left_frame", "past_far", "hit_first", "hit_later", "thick_reject",
            "bias_reject", "refine_moved", "no_hit", "edge_faded", "length_faded", "k_zero")
# the status word of the checker's debug plane
ST_SKY, ST_ROUGH, ST_BEHIND_NEAR, ST_LEFT_FRAME, ST_PAST_FAR, ST_EXHAUSTED, ST_HIT = range(7)
DEFAULTS = dict(maxDistance=20.0, thickness=0.5, bias=0.02, maxRoughness=0.75, steps=32, edgeFade=32, intensity=256)
# the parameter sets of the corpus: every N of {1, 2, 32, 63, 64};
#   short_n1    one sample 5 units along the ray
#   thick_n2    two samples, a thickness that accepts most of what lies behind a surface, a narrow edge fade
#   long_n63    rays that reach the far plane, no bias, half intensity, the widest edge fade
#   mirror_n64  the mirror anchor's: every surface reflects, anything behind a surface is a hit
PARAM_SETS = {
    "default": DEFAULTS,
    "short_n1": dict(DEFAULTS, maxDistance=5.0, steps=1),
    "thick_n2": dict(DEFAULTS, thickness=8.0, steps=2, edgeFade=4),
    "long_n63": dict(DEFAULTS, maxDistance=120.0, bias=0.0, steps=63, edgeFade=1024, intensity=128),
    "mirror_n64": dict(DEFAULTS, maxDistance=30.0, thickness=50.0, bias=0.001, steps=64, edgeFade=4),
}
# the fog's sizes: widths +- 1 of a multiple of the kernel's 32 x 8 workgroup (four 8 x 8 wavefront tiles), heights either side of 8,
# degenerate frames, and one frame of several workgroups each way
SIZES = fog_lib.SIZES
DEPTH_KINDS = ("zeros", "ones", "random", "ramp")


def build():
    return build_checker(SRC, LIB)


def params_array(params=None):
    """The eight words of crychic_ssr_params: what ssr_ref and ssh_ssr take."""
    p = dict(DEFAULTS, **(params or {}))
    f = np.array([p["maxDistance"], p["thickness"], p["bias"], p["maxRoughness"]], np.float32).view(np.uint32)
    return np.array(list(f) + [p["steps"], p["edgeFade"], p["intensity"], 0], np.uint32)


class Frame:
    """What the pass reads besides the image: Proj, ViewProj, InvViewProj (16 floats each, stored transposed), EyePosW, NearZ, the
    (H, W) uint32 depth plane and the three (H, W, 4) float32 G-buffer planes (what a half4 plane widens to)."""

    def __init__(self, proj, vp, ivp, eye, nearZ, g0, g1, g2, depth):
        self.proj, self.vp, self.ivp = (np.ascontiguousarray(m, np.float32).reshape(16).copy() for m in (proj, vp, ivp))
        self.eye = np.ascontiguousarray(eye, np.float32).reshape(3).copy()
        self.nearZ = np.array([nearZ], np.float32)
        self.depth = np.ascontiguousarray(depth, np.uint32)
        self.g = [np.ascontiguousarray(g, np.float32) for g in (g0, g1, g2)]
        H, W = self.depth.shape
        assert all(g.shape == (H, W, 4) for g in self.g)

    @classmethod
    def from_pass_cb(cls, pcb, g0, g1, g2, depth):
        """pcb: a PassConstants (any ctypes object or buffer of its 2048 bytes)."""
        f = np.frombuffer(bytes(pcb), np.float32)
        # float offsets in crychic_pass_constants: Proj 32, ViewProj 64, InvViewProj 80, EyePosW 304, NearZ 312
        return cls(f[32:48], f[64:80], f[80:96], f[304:307], f[312], g0, g1, g2, depth)

    def with_(self, **kw):
        """A copy with the named fields replaced (proj, vp, ivp, eye, nearZ, g0, g1, g2, depth)."""
        cur = dict(proj=self.proj, vp=self.vp, ivp=self.ivp, eye=self.eye, nearZ=self.nearZ[0], g0=self.g[0], g1=self.g[1], g2=self.g[2],
                   depth=self.depth)
        cur.update(kw)
        return Frame(**cur)

    def pass_constants(self, lib):
        """A PassConstants of the product's bindings holding this frame's fields (the rest zero)."""
        pcb = lib.PassConstants()
        f = np.zeros(C.sizeof(pcb) // 4, np.float32)
        f[32:48], f[64:80], f[80:96], f[304:307], f[312] = self.proj, self.vp, self.ivp, self.eye, self.nearZ[0]
        C.memmove(C.addressof(pcb), f.ctypes.data, C.sizeof(pcb))
        return pcb

    def plane(self, k, mix=0):
        """G-buffer plane k as the call with format mix `mix` (bit k: half4) takes it.  A half plane exists only where every value
        of the float plane is a half's."""
        if not (mix >> k) & 1:
            return self.g[k]
        h = self.g[k].astype(np.float16)
        assert np.array_equal(h.astype(np.float32).view(np.uint32), self.g[k].view(np.uint32)), "plane %d does not hold halves" % k
        return h


def format_flags(mix):
    """The CRYCHIC_GBUFFER_G*_F16 bits of format mix 0 .. 7."""
    return mix << 12


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.ssr_ref.argtypes = [C.c_void_p] * 11 + [C.c_uint32] * 4 + [C.c_void_p] * 3
        _REF.ssr_ref.restype = None
    return _REF


def checker(frame, img, params=None, row0=0, rows=None, out=None):
    """(rows [row0, row0 + rows) of the (H, W, 4) uint8 frame `img` with its reflections, written into `out` -- a frame of 0xA5 by
    default --, {counter: count over those rows}, the (H, W, 4) int32 debug plane { status, hx, hy, tq } -- -1 outside the rows)."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    assert frame.depth.shape == (H, W)
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    n = np.zeros(len(COUNTERS), np.uint64)
    dbg = np.full((H, W, 4), -1, np.int32)
    p = params_array(params)
    _ref().ssr_ref(frame.proj.ctypes.data, frame.vp.ctypes.data, frame.ivp.ctypes.data, frame.eye.ctypes.data, frame.nearZ.ctypes.data,
                   frame.g[0].ctypes.data, frame.g[1].ctypes.data, frame.g[2].ctypes.data, frame.depth.ctypes.data, img.ctypes.data, out.ctypes.data,
                   W, H, row0, rows, p.ctypes.data, n.ctypes.data, dbg.ctypes.data)
    return out, dict(zip(COUNTERS, (int(v) for v in n))), dbg


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

def camera_constants(W, H, cam=None):
    return fog_lib.camera_constants(W, H, 16, cam=cam)


def make_depth(kind, W, H, rng):
    if kind == "zeros":
        return np.zeros((H, W), np.uint32)
    if kind == "ones":
        return np.full((H, W), 0xFFFFFF, np.uint32)
    if kind == "random":
        return rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)                # 24 random bits and a random top byte
    # a ramp in view depth from 3 units at the bottom row to 60 at the top (a floor seen from above), with a random top byte, a few
    # columns 2 units nearer (posts for the rays to meet) and a few sky texels
    z = np.linspace(60.0, 3.0, H)[:, None] * np.ones((1, W))
    z[:, ::5] -= 2.0
    A, B = 100.0 / 99.0, -100.0 / 99.0
    d = np.round(np.clip(A + B / z, 0.0, 1.0) * 16777215.0).astype(np.uint32)
    d[rng.random((H, W)) < 0.05] = 0xFFFFFF
    return d | (rng.integers(0, 256, (H, W), dtype=np.uint32) << 24)


def random_gbuffer(W, H, rng, halves=False):
    """Random planes: normals over [-1, 1]^3, albedo, roughness and metalness over [0, 1] (a quarter of the texels too rough for
    the default maxRoughness); halves: every value a half's."""
    g0 = rng.uniform(-30.0, 30.0, (H, W, 4)).astype(np.float32)
    g0[..., 3] = rng.random((H, W))
    g1 = rng.random((H, W, 4)).astype(np.float32)
    g2 = rng.uniform(-1.0, 1.0, (H, W, 4)).astype(np.float32)
    if halves:
        g0, g1, g2 = (g.astype(np.float16).astype(np.float32) for g in (g0, g1, g2))
    return g0, g1, g2


def floor_gbuffer(W, H, rng):
    """Planes of a floor: normals near straight up, smooth and metallic, albedo random."""
    g0, g1, g2 = random_gbuffer(W, H, rng)
    g2[..., :3] = (0.0, 1.0, 0.0)
    g2[..., :3] += rng.uniform(-0.05, 0.05, (H, W, 3)).astype(np.float32)
    g1[..., 3] *= 0.5
    return g0, g1, g2


def golden_frame():
    """The committed 64 x 64 frame with its roughness scaled by a quarter, so that the floor reflects well, and the frame lit from
    the unscaled planes."""
    g = np.load(GOLD, allow_pickle=False)
    g1 = np.array(g["g1"])
    g1[..., 3] *= 0.25
    return Frame.from_pass_cb(g["pass_cb"].tobytes(), g["g0"], g1, g["g2"], g["depth"]), np.ascontiguousarray(g["lit_3light_intended_sky"])


_SCENE = {}


def scene_frame():
    """The 128 x 96 synthetic scene (crychic_renderer_amd.scene, on the CPU) with its roughness scaled by a quarter."""
    if "frame" not in _SCENE:
        from crychic_renderer_amd import scene
        planes = scene.make_scene(128, 96, shadow_dim=16, cube_dim=8, device="cpu")
        g1 = planes["g1"].numpy().copy()
        g1[..., 3] *= 0.25
        _SCENE["frame"] = Frame.from_pass_cb(planes["consts"].pass_cb, planes["g0"].numpy(), g1, planes["g2"].numpy(),
                                             planes["depth"].numpy().view(np.uint32))
    return _SCENE["frame"]


WALL_Z = 5.0
FLOOR_COLOUR = (10, 20, 30, 200)


def mirror_scene(W, H):
    """The anchor's scene under the reference camera, by float64 ray casting: the floor y = 0 (normal up, roughness 0, metalness 1,
    albedo 1) in front of the wall z = WALL_Z, which faces the camera, does not reflect and whose colour encodes its pixel's
    coordinates.  Returns (Frame, image, truth) with truth a dict of (H, W) float64 planes for the floor pixels: `floor` (bool),
    `tx`, `ty` the projection in pixels of the point where the pixel's mirrored ray meets the wall, `length` of that ray in world units
    and `stride` the screen length in pixels of the whole ray of PARAM_SETS["mirror_n64"] divided by its N."""
    from crychic_renderer_amd import scene
    cam = scene.default_camera(W, H)
    ex, ey, ez = (float(v) for v in cam.pos)
    assert tuple(cam.look) == (0.0, 0.0, 1.0) and tuple(cam.up) == (0.0, 1.0, 0.0)
    th = math.tan(0.5 * cam.fovY)
    aspect = float(cam.aspect)
    xs = (np.arange(W) + 0.5) / W * 2.0 - 1.0
    ys = 1.0 - (np.arange(H) + 0.5) / H * 2.0
    dx = np.broadcast_to((xs * aspect * th)[None, :], (H, W))
    dy = np.broadcast_to((ys * th)[:, None], (H, W))
    wall_view = WALL_Z - ez
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = np.where(dy < 0, -ey / dy, np.inf)            # view depth of the floor along the pixel's ray (its z component is 1)
    floor = tf < wall_view
    zview = np.where(floor, tf, wall_view)
    A = cam.farZ / (cam.farZ - cam.nearZ)
    B = -cam.nearZ * cam.farZ / (cam.farZ - cam.nearZ)
    depth = np.round(np.clip(A + B / zview, 0.0, 1.0) * 16777215.0).astype(np.uint32)
    pos = np.stack([ex + zview * dx, ey + zview * dy, ez + zview], axis=-1)
    g0 = np.concatenate([pos, np.where(floor, 1.0, 0.0)[..., None]], axis=-1).astype(np.float32)
    g1 = np.ones((H, W, 4), np.float32)
    g1[..., 3] = np.where(floor, 0.0, 1.0)
    g2 = np.zeros((H, W, 4), np.float32)
    g2[..., 1] = np.where(floor, 1.0, 0.0)
    g2[..., 2] = np.where(floor, 0.0, -1.0)
    g2[..., 3] = 1.0
    img = np.zeros((H, W, 4), np.uint8)
    img[..., 0] = np.arange(W, dtype=np.uint8)[None, :]
    img[..., 1] = np.arange(H, dtype=np.uint8)[:, None]
    img[..., 2] = 0x40
    img[..., 3] = 255
    img[floor] = FLOOR_COLOUR
    frame = Frame.from_pass_cb(camera_constants(W, H), g0, g1, g2, depth)

    def project(p):
        vz = p[..., 2] - ez
        return (0.5 + 0.5 * (p[..., 0] - ex) / (vz * aspect * th)) * W, (0.5 - 0.5 * (p[..., 1] - ey) / (vz * th)) * H
    # the mirrored ray of a floor pixel: the view ray with its y component turned round
    r = np.stack([dx, -dy, np.ones((H, W))], axis=-1)
    r /= np.linalg.norm(r, axis=-1, keepdims=True)
    s = (WALL_Z - pos[..., 2]) / r[..., 2]
    tx, ty = project(pos + s[..., None] * r)
    x0, y0 = project(pos)
    x1, y1 = project(pos + PARAM_SETS["mirror_n64"]["maxDistance"] * r)
    stride = np.hypot(x1 - x0, y1 - y0) / PARAM_SETS["mirror_n64"]["steps"]
    return frame, img, dict(floor=floor, tx=tx, ty=ty, length=s, stride=stride)


def mirror_eligible(truth, W, H, params):
    """The floor pixels whose true mirrored ray meets the wall inside the frame, more than edgeFade from its border and within 3/4
    of maxDistance."""
    E = params["edgeFade"]
    tx, ty = truth["tx"], truth["ty"]
    return truth["floor"] & (tx > E + 1) & (tx < W - 1 - E) & (ty > E + 1) & (ty < H - 1 - E) & (truth["length"] <= 0.75 * params["maxDistance"])


def check_mirror(W, H, out, dbg, frame, img, truth):
    """The anchor's assertions on a frame `out` of the pass and the checker's debug plane."""
    p = PARAM_SETS["mirror_n64"]
    el = mirror_eligible(truth, W, H, p)
    assert el.sum() >= W * H // 8, "too few eligible pixels: %d" % el.sum()
    hit = dbg[..., 0] == ST_HIT
    assert (hit & el).sum() >= 0.9 * el.sum(), "%d of %d eligible pixels report a hit" % ((hit & el).sum(), el.sum())
    ys, xs = np.nonzero(hit & el)
    hx, hy, tq = (dbg[ys, xs, k].astype(np.int64) for k in (1, 2, 3))
    dist = np.hypot(hx + 0.5 - truth["tx"][ys, xs], hy + 0.5 - truth["ty"][ys, xs])
    bound = 1.0 + truth["stride"][ys, xs] / 16.0
    assert (dist <= bound).all(), "a hit pixel %.3f from the true hit's projection (bound %.3f)" % (dist.max(), bound[dist.argmax()])
    assert not truth["floor"][hy, hx].any(), "a hit on the floor"
    e = np.minimum(np.minimum(hx, W - 1 - hx), np.minimum(hy, H - 1 - hy))
    fe = np.minimum(e, p["edgeFade"]) * 65536 // p["edgeFade"]
    fd = np.minimum(65536, 4 * (65536 - tq))
    K = ((((65536 * fe) >> 16) * fd) >> 16) * p["intensity"] >> 8           # R0 = 1 and roughness 0: wq = 65536
    assert (fe == 65536).all()
    want = (img[ys, xs, :3].astype(np.int64) * (65536 - K)[:, None] + img[hy, hx, :3].astype(np.int64) * K[:, None] + 32768) >> 16
    assert np.array_equal(out[ys, xs, :3], want.astype(np.uint8)) and np.array_equal(out[..., 3], img[..., 3])
    # and what does not reflect is untouched
    assert np.array_equal(out[~truth["floor"]], img[~truth["floor"]])


_CORPUS = {}


def corpus():
    """[(name, Frame, image, parameter-set name, format mix)]: built once and read-only.  The rendered frames under every parameter
    set; every size of SIZES under combinations that between them take every depth kind and parameter set; the mirror scenes; a near
    plane far inside the scene; normals of zero length and non-finite entries in the G-buffer and in ViewProj; the eight format mixes
    of one frame; a very wide and a very tall frame."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    rng = np.random.default_rng(27)
    cases = []
    gold, lit = golden_frame()
    sc = scene_frame()
    sc_img = rng.integers(0, 256, (96, 128, 4), dtype=np.uint8)
    for pname in PARAM_SETS:
        cases.append(("golden64_" + pname, gold, lit, pname, 0))
        cases.append(("scene128_" + pname, sc, sc_img, pname, 0))
    for W, H in ((128, 96), (70, 38)):
        frame, img, _ = mirror_scene(W, H)
        cases.append(("mirror%dx%d" % (W, H), frame, img, "mirror_n64", 0))
    names = list(PARAM_SETS)
    for si, (W, H) in enumerate(SIZES + ((4100, 3), (3, 4100))):
        for v in range(4 if W * H < 10000 else 5):
            dk = DEPTH_KINDS[(si + v) % 4]
            pname = names[(2 * si + v) % 5]
            g0, g1, g2 = floor_gbuffer(W, H, rng) if dk == "ramp" else random_gbuffer(W, H, rng)
            frame = Frame.from_pass_cb(camera_constants(W, H), g0, g1, g2, make_depth(dk, W, H, rng))
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            cases.append(("%dx%d_%s_%s" % (W, H, dk, pname), frame, img, pname, 0))
    # the scene with the near plane 25 units out: nearer pixels are behind it, and rays towards the eye are cut at it
    cases.append(("scene128_near25", sc.with_(nearZ=25.0), sc_img, "long_n63", 0))
    W, H = 65, 7
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    base = Frame.from_pass_cb(camera_constants(W, H), *floor_gbuffer(W, H, rng), make_depth("ramp", W, H, rng))
    g2 = base.g[2].copy()
    g2[:, ::3, :3] = 0.0
    cases.append(("normals_zero", base.with_(g2=g2), img, "thick_n2", 0))
    bad = [g.copy() for g in base.g]
    for k, g in enumerate(bad):
        g[k::3, 0::7] = np.nan
        g[k::3, 1::7] = np.inf
        g[k::3, 2::7] = -np.inf
        g[k::3, 3::7, 3] = -1.0e38
    cases.append(("gbuffer_nonfinite", base.with_(g0=bad[0], g1=bad[1], g2=bad[2]), img, "default", 0))
    for tag, edits in (("inf", {0: np.inf, 5: -np.inf}), ("nan", {10: np.nan}), ("w_inf", {15: np.inf}), ("w_zero", {12: 0, 13: 0, 14: 0, 15: 0})):
        vp = base.vp.copy()
        for k, val in edits.items():
            vp[k] = val
        cases.append(("vp_" + tag, base.with_(vp=vp), img, "default", 0))
    W, H = 130, 9
    fm = Frame.from_pass_cb(camera_constants(W, H), *(g.astype(np.float16).astype(np.float32) for g in floor_gbuffer(W, H, rng)),
                            make_depth("ramp", W, H, rng))
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    for mix in range(8):
        cases.append(("130x9_formats_%d" % mix, fm, img, "thick_n2", mix))
    for _, frame, im, _, _ in cases:
        for arr in [frame.proj, frame.vp, frame.ivp, frame.eye, frame.nearZ, frame.depth, im] + frame.g:
            arr.setflags(write=False)
    _CORPUS["cases"] = cases
    return cases


_EXPECTED = {}


def expected(name):
    """The checker's whole frame, counters and debug plane for corpus case `name`; computed once, read-only."""
    if name not in _EXPECTED:
        case = {c[0]: c for c in corpus()}[name]
        out, n, dbg = checker(case[1], case[2], PARAM_SETS[case[3]])
        out.setflags(write=False)
        dbg.setflags(write=False)
        _EXPECTED[name] = (out, n, dbg)
    return _EXPECTED[name]
