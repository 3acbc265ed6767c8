"""Builds and loads tests/ssr_gloss_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_ssr_pyramid and crychic_ssr_glossy, plain C
written from the definition in include/crychic_hip.h with none of the kernels' code; the gloss settings the host and the device tests
run the corpus of ssr_lib under; the frames of the pyramid's own tests; and the level anchor on ssr_lib's mirror scene."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, build_checker
import ssr_lib as sl

ROOT = sl.ROOT
DIR = os.path.join(ROOT, "tests", "ssr_gloss_ref")
SRC, LIB = os.path.join(DIR, "ssr_gloss_ref.c"), os.path.join(DIR, "libssrglossref.so")

MAX_LEVELS = 8
COUNTERS = sl.COUNTERS + ("lq_zero", "lq_positive", "f_zero", "f_positive", "k_neff", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom")
# the branches of 6a and 6b that the corpus must take between the three settings
BRANCHES = ("lq_zero", "lq_positive", "f_zero", "f_positive", "k_neff", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom")
GLOSS_DEFAULTS = dict(coneScale=0.0, levels=6)      # coneScale 0: profiles/ssr_gloss_quality.txt
GLOSS_SETS = {
    "default": GLOSS_DEFAULTS,
    "c05_l3": dict(coneScale=0.5, levels=3),
    "c16_l8": dict(coneScale=16.0, levels=8),
}
# the pyramid's sizes: one texel, a line, one workgroup's tile and its neighbours either way (a destination tile is 32 x 16), widths
# that are and are not multiples of four (the 16-byte loads), and frames thin enough for one side to reach 1 long before the other
PYRAMID_SIZES = ((1, 1), (1, 7), (2, 2), (3, 5), (33, 17), (65, 34), (130, 70), (4100, 3), (3, 4100), (65600, 2))


def build():
    return build_checker(SRC, LIB)


def gloss_array(gloss=None):
    """The four words of crychic_ssr_gloss_params."""
    g = dict(GLOSS_DEFAULTS, **(gloss or {}))
    return np.array([np.array([g["coneScale"]], np.float32).view(np.uint32)[0], g["levels"], 0, 0], np.uint32)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.ssr_gloss_plan_ref.argtypes = [C.c_uint32] * 3 + [C.c_void_p]
        _REF.ssr_gloss_plan_ref.restype = C.c_uint32
        _REF.ssr_gloss_pyramid_ref.argtypes = [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p]
        _REF.ssr_gloss_pyramid_ref.restype = None
        _REF.ssr_gloss_ref.argtypes = [C.c_void_p] * 12 + [C.c_uint32] * 4 + [C.c_void_p] * 4
        _REF.ssr_gloss_ref.restype = None
    return _REF


def plan(W, H, levels):
    """(n_eff, [(W_k, H_k, byte offset) for k = 0 .. n_eff], workspace bytes) by the checker."""
    sizes = np.zeros(3 * MAX_LEVELS + 1, np.uint64)
    n = _ref().ssr_gloss_plan_ref(W, H, levels, sizes.ctypes.data)
    return n, [tuple(int(v) for v in sizes[3 * k:3 * k + 3]) for k in range(n + 1)], int(sizes[-1])


def level_views(workspace, W, H, levels):
    """[None, level 1, .. level n_eff]: (H_k, W_k, 4) uint8 views into the flat uint8 array `workspace`."""
    n, sizes, _ = plan(W, H, levels)
    return [None] + [workspace[o:o + w * h * 4].reshape(h, w, 4) for w, h, o in sizes[1:]]


def pyramid(img, levels, workspace=None):
    """The checker's pyramid of the (H, W, 4) uint8 frame `img`: a flat uint8 array of at least 16 bytes, GUARD wherever no level
    lies, or `workspace` written in place."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    if workspace is None:
        workspace = np.full(max(plan(W, H, levels)[2], 16), GUARD, np.uint8)
    _ref().ssr_gloss_pyramid_ref(img.ctypes.data, W, H, levels, workspace.ctypes.data)
    return workspace


def checker(frame, img, params=None, gloss=None, row0=0, rows=None, out=None, pyr=None):
    """As ssr_lib.checker for crychic_ssr_glossy: (out, counters, the (H, W, 8) int32 debug plane { status, hx, hy, tq, lq, R, G, B }).
    pyr: the pyramid to read, by default the checker's own of `img`."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    assert frame.depth.shape == (H, W)
    g = gloss_array(gloss)
    pyr = pyramid(img, int(g[1])) if pyr is None else pyr
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    n = np.zeros(len(COUNTERS), np.uint64)
    dbg = np.full((H, W, 8), -1, np.int32)
    p = sl.params_array(params)
    _ref().ssr_gloss_ref(frame.proj.ctypes.data, frame.vp.ctypes.data, frame.ivp.ctypes.data, frame.eye.ctypes.data, frame.nearZ.ctypes.data,
                         frame.g[0].ctypes.data, frame.g[1].ctypes.data, frame.g[2].ctypes.data, frame.depth.ctypes.data, img.ctypes.data,
                         pyr.ctypes.data, out.ctypes.data, W, H, row0, rows, p.ctypes.data, g.ctypes.data, n.ctypes.data, dbg.ctypes.data)
    return out, dict(zip(COUNTERS, (int(v) for v in n))), dbg


_EXPECTED = {}


def expected(name, gname):
    """The checker's pyramid, whole frame, counters and debug plane for case `name` of ssr_lib.corpus() under GLOSS_SETS[gname];
    computed once, read-only."""
    key = (name, gname)
    if key not in _EXPECTED:
        case = {c[0]: c for c in sl.corpus()}[name]
        pyr = pyramid(case[2], GLOSS_SETS[gname]["levels"])
        out, n, dbg = checker(case[1], case[2], sl.PARAM_SETS[case[3]], GLOSS_SETS[gname], pyr=pyr)
        for a in (pyr, out, dbg):
            a.setflags(write=False)
        _EXPECTED[key] = (pyr, out, n, dbg)
    return _EXPECTED[key]


# ---- the pyramid's frames ---------------------------------------------------------------------------------------------------------

def pyramid_frame(W, H, seed=31):
    return np.random.default_rng(seed + 7 * W + H).integers(0, 256, (H, W, 4), dtype=np.uint8)


def affine_frame(W, H):
    """R = x, G = y (W, H <= 255), B their sum halved, A = 255 - x."""
    assert W <= 255 and H <= 255
    img = np.zeros((H, W, 4), np.uint8)
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    img[..., 0], img[..., 1], img[..., 2], img[..., 3] = x, y, (x + y) // 2, 255 - x
    return img


def check_affine(W, H, views):
    """The definition's affine answer on R and G of the levels `views` (level_views) of affine_frame(W, H): a level-k texel whose
    level-0 support -- 4 * 2^k - 3 columns and rows about its centre (2^k (x + 1/2) - 1/2) -- lies inside the frame is within k / 2 of
    the affine value there.  Each level rounds by at most 1/2 and the filter is a convex combination that reproduces affine
    functions.  Returns the number of texels checked."""
    checked = 0
    for k in range(1, len(views)):
        hk, wk = views[k].shape[:2]
        half = (4 * 2 ** k - 3 - 1) / 2.0
        cx = 2 ** k * (np.arange(wk) + 0.5) - 0.5
        cy = 2 ** k * (np.arange(hk) + 0.5) - 0.5
        okx = (cx - half >= 0) & (cx + half <= W - 1)
        oky = (cy - half >= 0) & (cy + half <= H - 1)
        sel = oky[:, None] & okx[None, :]
        errR = np.abs(views[k][..., 0].astype(np.float64) - cx[None, :])[sel]
        errG = np.abs(views[k][..., 1].astype(np.float64) - cy[:, None])[sel]
        assert (errR <= k / 2.0).all() and (errG <= k / 2.0).all(), "level %d: off the affine value by %.3f (bound %.1f)" % (
            k, max(errR.max(initial=0), errG.max(initial=0)), k / 2.0)
        checked += int(sel.sum())
    return checked


def check_pyramid_answers(build_levels):
    """The definition's known answers of the pyramid on `build_levels(img, levels)` -> level_views of the pyramid under test."""
    rng = np.random.default_rng(5)
    # one colour: every texel of every level
    img = np.empty((37, 70, 4), np.uint8)
    img[:] = (13, 255, 0, 97)
    for lv in build_levels(img, 8)[1:]:
        assert (lv == img[0, 0]).all()
    # transposing the frame transposes every level
    img = rng.integers(0, 256, (45, 83, 4), dtype=np.uint8)
    a, b = build_levels(img, 8), build_levels(np.ascontiguousarray(img.transpose(1, 0, 2)), 8)
    assert len(a) == len(b) == 8
    for la, lb in zip(a[1:], b[1:]):
        assert np.array_equal(la.transpose(1, 0, 2), lb)
    # columns alternating 0 and 255: 128 in every level-1 texel whose four source columns are unclamped
    img = np.zeros((9, 70, 4), np.uint8)
    img[:, 1::2] = 255
    l1 = build_levels(img, 2)[1]
    assert l1.shape == (5, 35, 4) and (l1[:, 1:34] == 128).all()
    # affine
    for W, H in ((255, 200), (130, 70)):
        assert check_affine(W, H, build_levels(affine_frame(W, H), 8)) > 1000


# ---- the level anchor -------------------------------------------------------------------------------------------------------------

ANCHOR_GLOSS = dict(coneScale=0.5, levels=8)
ANCHOR_ROUGH = 0.5


def anchor_scene(W, H, rough=ANCHOR_ROUGH):
    """ssr_lib.mirror_scene with the floor's roughness `rough`: (Frame, image, truth)."""
    frame, img, truth = sl.mirror_scene(W, H)
    g1 = frame.g[1].copy()
    g1[..., 3] = np.where(truth["floor"], np.float32(rough), np.float32(1.0))
    return frame.with_(g1=g1), img, truth


def check_level_anchor(W, H, dbg, truth):
    """The anchor's assertions on the debug plane of the pass over anchor_scene(W, H) under PARAM_SETS["mirror_n64"] and ANCHOR_GLOSS:
    on the eligible pixels whose true r = coneScale rough L_true >= 2, L_true the float64 screen distance from the pixel's centre to
    the true hit's projection, lq is within 256 log2(1 + (1.71 + stride / 16) / L_true) + 2 of 256 log2(r): the existing anchor's
    hit bound (1 + stride / 16) plus half a pixel's diagonal (0.71), plus rounding."""
    p = sl.PARAM_SETS["mirror_n64"]
    ys, xs = np.mgrid[0:H, 0:W]
    L = np.hypot(truth["tx"] - (xs + 0.5), truth["ty"] - (ys + 0.5))
    with np.errstate(invalid="ignore"):
        r = ANCHOR_GLOSS["coneScale"] * ANCHOR_ROUGH * L
        sel = sl.mirror_eligible(truth, W, H, p) & (r >= 2.0)
    assert sel.sum() >= W * H // 8, "too few anchor pixels: %d of %d" % (sel.sum(), W * H)
    hit = dbg[..., 0] == sl.ST_HIT
    assert (hit & sel).sum() >= 0.9 * sel.sum(), "%d of %d anchor pixels report a hit" % ((hit & sel).sum(), sel.sum())
    m = hit & sel
    want = 256.0 * np.log2(r[m])
    bound = 256.0 * np.log2(1.0 + (1.71 + truth["stride"][m] / 16.0) / L[m]) + 2.0
    err = np.abs(dbg[..., 4][m] - want)
    print("level anchor %dx%d: %d pixels (%.1f %% of the frame), levels up to %.2f, worst |lq - 256 log2 r| %.2f at bound %.2f" % (
        W, H, sel.sum(), 100.0 * sel.sum() / (W * H), want.max() / 256.0, err.max(), bound[err.argmax()]))
    assert (err <= bound).all(), "lq %.2f from 256 log2(r) (bound %.2f)" % (err.max(), bound[err.argmax()])
