"""Builds and loads tests/bloom_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_bloom, plain C written from the definition in
include/crychic_hip.h with none of the kernels' code; a Python restatement of the workspace layout; and the corpus of frames and
parameter sets the host and the device tests share."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "bloom_ref")
SRC, LIB = os.path.join(DIR, "bloom_ref.c"), os.path.join(DIR, "libbloomref.so")

COUNTERS = ("w_zero", "w_interior", "w_full", "clamp_down", "clamp_up", "saturated")
MAX_LEVELS = 8
DEFAULTS = dict(threshold=192, knee=32, scatter=179, intensity=128, levels=6)
FIELDS = ("threshold", "knee", "scatter", "intensity", "levels")
# every end of every range, and middles; "dark" puts the threshold over every luma (L <= 65280 = 256 * 255)
PARAM_SETS = {
    "default": DEFAULTS,
    "one_level": dict(threshold=100, knee=1, scatter=179, intensity=256, levels=1),
    "eight_levels": dict(threshold=128, knee=255, scatter=256, intensity=1024, levels=8),
    "no_scatter": dict(threshold=64, knee=16, scatter=0, intensity=512, levels=4),
    "no_intensity": dict(threshold=0, knee=32, scatter=128, intensity=0, levels=6),
    "low_threshold": dict(threshold=0, knee=100, scatter=200, intensity=300, levels=3),
    "dark": dict(threshold=255, knee=32, scatter=179, intensity=128, levels=6),
    "two_levels": dict(threshold=160, knee=64, scatter=77, intensity=700, levels=2),
}
# the smallest sizes at which indexing can go wrong, then one either side of the downsample kernel's 32 x 16 destination tile
# (64 x 32 source texels): an exact fit and one texel over it both ways
SIZES = ((1, 1), (2, 3), (7, 5), (33, 17), (64, 64), (65, 63), (129, 97), (322, 190), (64, 32), (66, 34))


def build():
    return build_checker(SRC, LIB, fp=False)


# ---- the layout, restated ---------------------------------------------------------------------------------------------------------

def level_count(W, H, levels):
    m, lg = max(W, H), 0
    while (1 << lg) < m:
        lg += 1
    return min(levels, max(1, lg))


def level_sizes(W, H, levels):
    """[(W_k, H_k)] for k = 1 .. n_eff."""
    out = []
    for _ in range(level_count(W, H, levels)):
        W, H = (W + 1) >> 1, (H + 1) >> 1
        out.append((W, H))
    return out


def level_offsets(W, H, levels):
    """([offset of level k for k = 1 .. n_eff], workspace bytes)."""
    offs, at, end = [], 0, 0
    for w, h in level_sizes(W, H, levels):
        offs.append(at)
        end = at + w * h * 8
        at = (end + 15) & ~15
    return offs, end


def split_workspace(ws, W, H, levels):
    """The levels of the workspace bytes `ws` (a uint8 array) as [(H_k, W_k, 4) uint16 views]."""
    offs, _ = level_offsets(W, H, levels)
    return [ws[o:o + w * h * 8].view(np.uint16).reshape(h, w, 4) for o, (w, h) in zip(offs, level_sizes(W, H, levels))]


def written_mask(W, H, levels, nbytes):
    """A boolean array over `nbytes` workspace bytes: True where a level lies."""
    m = np.zeros(nbytes, bool)
    offs, _ = level_offsets(W, H, levels)
    for o, (w, h) in zip(offs, level_sizes(W, H, levels)):
        m[o:o + w * h * 8] = True
    return m


# ---- the checker ------------------------------------------------------------------------------------------------------------------

_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.bloom_ref.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 4 + [C.c_void_p] * 3
        _REF.bloom_ref.restype = C.c_uint32
        _REF.bloom_ref_levels.argtypes = [C.c_uint32] * 3
        _REF.bloom_ref_levels.restype = C.c_uint32
    return _REF


def params_array(params=None):
    p = dict(DEFAULTS, **(params or {}))
    return np.array([p[f] for f in FIELDS], np.uint32)


def checker(img, params=None, row0=0, rows=None, out=None, downs=False):
    """(rows [row0, row0 + rows) of the frame behind the pass over the (H, W, 4) uint8 `img`, written into `out` -- a frame of 0xA5 by
    default --, [U_k as (H_k, W_k, 4) uint16 for k = 1 .. n_eff], {counter: count}); with downs=True a fourth value, [D_k]."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    p = params_array(params)
    sizes = level_sizes(W, H, int(p[4]))
    U = [np.zeros((h, w, 4), np.uint16) for w, h in sizes]
    D = [np.zeros((h, w, 4), np.uint16) for w, h in sizes]
    up = (C.c_void_p * MAX_LEVELS)(*[a.ctypes.data for a in U])
    dp = (C.c_void_p * MAX_LEVELS)(*[a.ctypes.data for a in D])
    n = np.zeros(len(COUNTERS), np.uint64)
    got = _ref().bloom_ref(p.ctypes.data, img.ctypes.data, out.ctypes.data, W, H, row0, rows, up, dp, n.ctypes.data)
    assert got == len(sizes), "the checker and the Python restatement disagree on n_eff"
    counts = dict(zip(COUNTERS, (int(v) for v in n)))
    return (out, U, counts, D) if downs else (out, U, counts)


# ---- the corpus -------------------------------------------------------------------------------------------------------------------

def corner_blob(W, H, rng, corner):
    """A random dim frame with a saturated blob at one frame corner (0 .. 3: top left, top right, bottom left, bottom right)."""
    img = rng.integers(0, 120, (H, W, 4), dtype=np.uint8)
    bw, bh = max(1, W // 3), max(1, H // 3)
    ys = slice(0, bh) if corner < 2 else slice(H - bh, H)
    xs = slice(0, bw) if corner % 2 == 0 else slice(W - bw, W)
    img[ys, xs, :3] = rng.integers(230, 256, img[ys, xs, :3].shape, dtype=np.uint8)
    return img


_SCENE = {}


def scene_frame():
    """The 128 x 96 synthetic scene lit on the CPU by the host build of the lighting kernel (three lights, sky): RGBA8."""
    if "img" not in _SCENE:
        import hostsim_lib
        import scene_util
        pl = scene_util.cpu_scene(128, 96, 256, 32)
        img, _ = hostsim_lib.load().light_frame(pl["consts"].pass_cb, scene_util.np_planes(pl), None, 3, 0.0, 1)
        img = np.ascontiguousarray(img)
        img.setflags(write=False)
        _SCENE["img"] = img
    return _SCENE["img"]


# The scene's sky and lit faces lie over luma 192, so the defaults change it (the tests assert that with the checker); this is the second
# set its tests use, to show that a caller's parameters reach the pass.  Both leave most of the frame unsaturated, so that the
# anti-aliasing behind the pass still finds edges.
SCENE_PARAMS = dict(threshold=160, knee=32, scatter=179, intensity=64, levels=6)

_CORPUS = {}


def corpus():
    """[(name, image, parameter-set name)]: built once and read-only.  Every size as noise and with a corner blob, the parameter sets
    taken in turn; the rendered scene under every parameter set."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    rng = np.random.default_rng(23)
    names = list(PARAM_SETS)
    cases = []
    turn = 0
    for W, H in SIZES:
        for kind in ("noise", "blob"):
            pname = names[turn % len(names)]
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8) if kind == "noise" else corner_blob(W, H, rng, turn % 4)
            cases.append(("%dx%d_%s_%s" % (W, H, kind, pname), img, pname))
            turn += 3                                           # 3 and 8 are coprime: the sets go round
    for pname in names:
        cases.append(("scene128_" + pname, scene_frame(), pname))
    cases.append(("scene128_scene", scene_frame(), "scene"))
    # more levels asked for than the frame has, on frames of more than one texel
    cases.append(("7x5_noise_deep", rng.integers(0, 256, (5, 7, 4), dtype=np.uint8), "eight_levels"))
    cases.append(("322x190_blob_default", corner_blob(322, 190, rng, 3), "default"))
    for _, im, _ in cases:
        im.setflags(write=False)
    _CORPUS["cases"] = cases
    return cases


def case_params(pname):
    return SCENE_PARAMS if pname == "scene" else PARAM_SETS[pname]


_EXPECTED = {}


def expected(name):
    """The checker's (frame, [U_k], counters) for corpus case `name`; computed once, read-only."""
    if name not in _EXPECTED:
        case = {c[0]: c for c in corpus()}[name]
        out, U, n = checker(case[1], case_params(case[2]))
        out.setflags(write=False)
        for u in U:
            u.setflags(write=False)
        _EXPECTED[name] = (out, U, n)
    return _EXPECTED[name]
