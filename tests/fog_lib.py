"""Builds and loads tests/fog_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_fog, plain C written from the definition in
include/crychic_hip.h with none of the kernel's code; and the corpus of frames, images and parameter sets the host and the device
tests share."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "fog_ref")
SRC, LIB = os.path.join(DIR, "fog_ref.c"), os.path.join(DIR, "libfogref.so")
GOLD = os.path.join(ROOT, "tests", "golden", "frame_64x64.npz")

COUNTERS = ("cascade0", "cascade1", "cascade2", "cascade3", "beyond", "outside", "lit", "shadowed", "lc_is_l", "lc_is_max", "qi_one", "qi_zero",
            "qi_between", "clamped", "mixed_run")
DEFAULTS = dict(density=0.02, maxDistance=100.0, steps=16, ambient=(70, 80, 100), sun=(150, 140, 110))
# the five parameter sets of the corpus: every N of {1, 2, 16, 63, 64};
#   thin_n1     so thin that qi rounds to 65536 for the nearest pixels and stays below it for the rest
#   far_n2      maxDistance 150: samples at t >= 100
#   bright_n63  in-scatter colours of 255: channels clamp at 255
#   dense_n64   density 16: qi = 0 for the distant pixels
PARAM_SETS = {
    "default": DEFAULTS,
    "thin_n1": dict(DEFAULTS, density=4e-6, maxDistance=40.0, steps=1),
    "far_n2": dict(DEFAULTS, density=0.01, maxDistance=150.0, steps=2),
    "bright_n63": dict(DEFAULTS, density=0.1, maxDistance=60.0, steps=63, ambient=(255, 255, 255), sun=(255, 250, 255)),
    "dense_n64": dict(DEFAULTS, density=16.0, steps=64),
}
# widths +- 1 of a multiple of the kernel's 32 x 8 workgroup (four 8 x 8 wavefront tiles), heights either side of 8, degenerate
# frames, and one frame of several workgroups each way
SIZES = ((1, 1), (3, 5), (63, 4), (64, 4), (65, 7), (130, 9), (322, 190))
MAP_SIDES = (1, 17, 100, 256)
DEPTH_KINDS = ("zeros", "ones", "random")
MAP_KINDS = ("zeros", "ones", "random", "step")


def build():
    return build_checker(SRC, LIB)


def params_array(params=None):
    """{ density bits, maxDistance bits, steps, ambient R G B, sun R G B } as nine uint32: what fog_ref and fgh_fog take."""
    p = dict(DEFAULTS, **(params or {}))
    f = np.array([p["density"], p["maxDistance"]], np.float32).view(np.uint32)
    return np.array([f[0], f[1], p["steps"]] + list(p["ambient"][:3]) + list(p["sun"][:3]), np.uint32)


class Frame:
    """What the pass reads besides the image: InvViewProj (16 floats, stored transposed), EyePosW, ShadowTransforms[0..3] (4 x 16,
    stored transposed), the (H, W) uint32 depth plane and the (4, dim, dim) uint32 cascade maps."""

    def __init__(self, ivp, eye, st, depth, maps):
        self.ivp = np.ascontiguousarray(ivp, np.float32).reshape(16).copy()
        self.eye = np.ascontiguousarray(eye, np.float32).reshape(3).copy()
        self.st = np.ascontiguousarray(st, np.float32).reshape(4, 16).copy()
        self.depth = np.ascontiguousarray(depth, np.uint32)
        self.maps = np.ascontiguousarray(maps, np.uint32)
        assert self.maps.ndim == 3 and self.maps.shape[0] == 4 and self.maps.shape[1] == self.maps.shape[2]
        self.dim = int(self.maps.shape[1])

    @classmethod
    def from_pass_cb(cls, pcb, depth, maps):
        """pcb: a PassConstants (any ctypes object or buffer of its 2048 bytes)."""
        f = np.frombuffer(bytes(pcb), np.float32)
        # float offsets in crychic_pass_constants: InvViewProj 80, ShadowTransforms 112, EyePosW 112 + 192
        return cls(f[80:96], f[304:307], f[112:176], depth, maps)

    def pass_constants(self, lib):
        """A PassConstants of the product's bindings holding this frame's three fields (the rest zero)."""
        pcb = lib.PassConstants()
        f = np.zeros(C.sizeof(pcb) // 4, np.float32)
        f[80:96], f[112:176], f[304:307] = self.ivp, self.st.reshape(64), self.eye
        C.memmove(C.addressof(pcb), f.ctypes.data, C.sizeof(pcb))
        return pcb


def map_pointers(frame):
    return (C.c_void_p * 4)(*[frame.maps[j].ctypes.data for j in range(4)])


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.fog_ref.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _REF.fog_ref.restype = None
    return _REF


def checker(frame, img, params=None, row0=0, rows=None, out=None, jitter=True, sums=False):
    """(rows [row0, row0 + rows) of the fogged (H, W, 4) uint8 frame `img` written into `out` -- a frame of 0xA5 by default --,
    {counter: count over those rows}); with sums=True a third value, the (H, W) uint32 plane of S (0 outside the rows)."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    assert frame.depth.shape == (H, W)
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    n = np.zeros(len(COUNTERS), np.uint64)
    S = np.zeros((H, W), np.uint32) if sums else None
    p = params_array(params)
    _ref().fog_ref(frame.ivp.ctypes.data, frame.eye.ctypes.data, frame.st.ctypes.data, frame.depth.ctypes.data, map_pointers(frame), frame.dim,
                   img.ctypes.data, out.ctypes.data, W, H, row0, rows, p.ctypes.data, 1 if jitter else 0, n.ctypes.data,
                   None if S is None else S.ctypes.data)
    counts = dict(zip(COUNTERS, (int(v) for v in n)))
    return (out, counts, S) if sums else (out, counts)


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

def camera_constants(W, H, dim, cam=None, light_dir=None):
    """The pass constants the library's own builders (crychic_update_cascade_shadow_transform, then crychic_update_main_pass_cb) make
    of the reference camera (or `cam`) for a W x H frame and dim x dim maps."""
    from crychic_renderer_amd import _lib, scene
    cam = cam or scene.default_camera(W, H)
    lv, lp, st = (np.zeros((4, 4, 4), np.float32) for _ in range(3))
    ld = (C.c_float * 3)(*(light_dir or scene.BASE_LIGHT_DIRS[0]))
    _lib.check(_lib.lib.crychic_update_cascade_shadow_transform(C.byref(cam), ld, dim, lv.ctypes.data, lp.ctypes.data, st.ctypes.data))
    pcb = _lib.PassConstants()
    dirs = np.asarray(scene.BASE_LIGHT_DIRS, np.float32)
    _lib.check(_lib.lib.crychic_update_main_pass_cb(C.byref(cam), W, H, st.ctypes.data, dirs.ctypes.data, C.byref(pcb)))
    return pcb


def make_depth(kind, W, H, rng):
    if kind == "zeros":
        return np.zeros((H, W), np.uint32)
    if kind == "ones":
        return np.full((H, W), 0xFFFFFF, np.uint32)
    return rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)                # 24 random bits and a random top byte


def make_maps(kind, dim, rng):
    if kind == "zeros":
        return np.zeros((4, dim, dim), np.uint32)
    if kind == "ones":
        return np.full((4, dim, dim), 0xFFFFFF, np.uint32)
    if kind == "random":
        return rng.integers(0, 1 << 32, (4, dim, dim), dtype=np.uint32)
    m = np.zeros((4, dim, dim), np.uint32)                                  # the half-plane step: 0 left of the middle column, 0xFFFFFF from it on
    m[:, :, dim // 2:] = 0xFFFFFF
    return m


def golden_frame():
    """The committed 64 x 64 frame: its depth plane, pass constants and rendered 64 x 64 cascades, and the frame lit from them."""
    g = np.load(GOLD, allow_pickle=False)
    return Frame.from_pass_cb(g["pass_cb"].tobytes(), g["depth"], g["shadow"]), np.ascontiguousarray(g["lit_3light_intended_sky"])


_SCENE = {}


def scene_frame():
    """The 128 x 96 synthetic scene with its rendered 256 x 256 cascades (crychic_renderer_amd.scene, on the CPU), and its planes."""
    if "frame" not in _SCENE:
        from crychic_renderer_amd import scene
        planes = scene.make_scene(128, 96, shadow_dim=256, cube_dim=8, device="cpu")
        _SCENE["frame"] = Frame.from_pass_cb(planes["consts"].pass_cb, planes["depth"].numpy().view(np.uint32), planes["shadow"].numpy().view(np.uint32))
    return _SCENE["frame"]


def straight_down_frame(W, H, dim, column):
    """The known-answer frame of a light straight down: the reference camera over a far-plane depth plane, every cascade with
    s.x = X / 100 + 0.5, s.y = Z / 100 + 0.5, s.z = 0.5 - Y / 50 (the light's depth grows downwards), and maps that are 0 (an occluder at
    the light: everything below is shadowed) left of texel column `column` and 0xFFFFFF (nothing in the way) from it on."""
    f = Frame.from_pass_cb(camera_constants(W, H, dim), np.full((H, W), 0xFFFFFF, np.uint32), np.zeros((4, dim, dim), np.uint32))
    one = np.array([0.01, 0, 0, 0.5, 0, 0, 0.01, 0.5, 0, -0.02, 0, 0.5, 0, 0, 0, 1], np.float32)
    f.st[:] = one
    f.maps[:, :, column:] = 0xFFFFFF
    return f


TIE_QI = 62960      # with N = 16: T_13 = 38912 and T_13 qi = 37382 * 65536 + 32768, so T_14 .. T_16 depend on the rounding constant


def tie_frame(W, H, dim):
    """The reference camera over a sphere around the eye: every pixel at the distance L at which the default parameters give
    qi == TIE_QI (the middle of that qi's range of L, about 32.08 units, where the range is 0.0135 units wide and a D24 step moves L by
    less than 0.0001), under maps with nothing in the way.  The depth words are found by bisection on a float64 reconstruction."""
    from post_restate import world_point64
    pcb = camera_constants(W, H, dim)
    frame = Frame.from_pass_cb(pcb, np.zeros((H, W), np.uint32), make_maps("ones", dim, None))
    per_unit = float(np.float32(DEFAULTS["density"]) * np.float32(1.44269504) / np.float32(DEFAULTS["steps"]))
    want = -np.log2(TIE_QI / 65536.0) / per_unit
    lo, hi = np.zeros((H, W), np.int64), np.full((H, W), 0xFFFFFF, np.int64)
    for _ in range(24):         # L grows with the depth word
        mid = (lo + hi) >> 1
        r = world_point64(frame.ivp, mid, W, H) - frame.eye.astype(np.float64)
        nearer = np.sqrt((r * r).sum(axis=-1)) < want
        lo, hi = np.where(nearer, mid, lo), np.where(nearer, hi, mid)
    return Frame(frame.ivp, frame.eye, frame.st, hi.astype(np.uint32), frame.maps)


_CORPUS = {}


def corpus():
    """[(name, Frame, image, parameter-set name, (depth kind, map kind))]: built once and read-only.  The rendered frames under every
    parameter set; every size of SIZES under combinations that between them take every map side, depth kind, map kind and parameter
    set; an eye far outside the cascades; non-finite entries in InvViewProj; the rounding tie of T."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    rng = np.random.default_rng(20)
    cases = []
    gold, lit = golden_frame()
    sc = scene_frame()
    sc_img = rng.integers(0, 256, (96, 128, 4), dtype=np.uint8)
    for pname in PARAM_SETS:
        cases.append(("golden64_" + pname, gold, lit, pname, ("rendered", "rendered")))
        cases.append(("scene128_" + pname, sc, sc_img, pname, ("rendered", "rendered")))
    names = list(PARAM_SETS)
    for si, (W, H) in enumerate(SIZES):
        for v in range(4 if W * H < 10000 else 5):
            dim = MAP_SIDES[(si + v) % 4]
            dk = DEPTH_KINDS[(si + 2 * v) % 3]
            mk = MAP_KINDS[(si + 3 * v + v // 4) % 4]
            pname = names[(2 * si + v) % 5]
            frame = Frame.from_pass_cb(camera_constants(W, H, dim), make_depth(dk, W, H, rng), make_maps(mk, dim, rng))
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            cases.append(("%dx%d_map%d_%s_%s_%s" % (W, H, dim, dk, mk, pname), frame, img, pname, (dk, mk)))
    W, H = 65, 7
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    base = Frame.from_pass_cb(camera_constants(W, H, 100), make_depth("random", W, H, rng), make_maps("random", 100, rng))
    far = Frame(base.ivp, (1.0e4, 1.0e4, -1.0e4), base.st, base.depth, base.maps)
    cases.append(("eye_far_outside", far, img, "far_n2", ("random", "random")))
    for tag, edits in (("inf", {0: np.inf, 5: -np.inf}), ("nan", {10: np.nan}), ("w_inf", {15: np.inf}), ("w_zero", {12: 0, 13: 0, 14: 0, 15: 0})):
        ivp = base.ivp.copy()
        for k, val in edits.items():
            ivp[k] = val
        cases.append(("ivp_" + tag, Frame(ivp, base.eye, base.st, base.depth, base.maps), img, "default", ("random", "random")))
    # the rounding of T (tests/test_post_restate_host.py, mutation t_round_32767): a constant of 32767 for 32768 shows only where
    # T_i qi is 32768 mod 65536, once in 65536 products, which no other case meets in a byte
    cases.append(("64x64_t_rounding_tie_default", tie_frame(64, 64, 17), rng.integers(0, 256, (64, 64, 4), dtype=np.uint8), "default",
                  ("rendered", "ones")))
    for _, frame, im, _, _ in cases:
        for arr in (frame.ivp, frame.eye, frame.st, frame.depth, frame.maps, im):
            arr.setflags(write=False)
    _CORPUS["cases"] = cases
    return cases


_EXPECTED = {}


def expected(name):
    """The checker's whole frame and counters for corpus case `name`; computed once, read-only."""
    if name not in _EXPECTED:
        case = {c[0]: c for c in corpus()}[name]
        out, n = checker(case[1], case[2], PARAM_SETS[case[3]])
        out.setflags(write=False)
        _EXPECTED[name] = (out, n)
    return _EXPECTED[name]
