"""Builds and loads tests/post_aa_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_antialias, plain C written from the definition
in include/crychic_hip.h with none of the kernel's code; and the corpus of images and parameter sets the host and the device tests
share."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "post_aa_ref")
SRC, LIB = os.path.join(DIR, "post_aa_ref.c"), os.path.join(DIR, "libpostaaref.so")
GOLD = os.path.join(ROOT, "tests", "golden", "frame_64x64.npz")

COUNTERS = ("early_copy", "horizontal", "vertical", "side_a", "side_b", "neg_hit", "neg_k", "pos_hit", "pos_k", "edge_wins", "subpix_wins",
            "zero_weight")
DEFAULTS = dict(absMin=2048, relShift=3, searchSteps=12, subpix=192)
# the parameter sets of the corpus: the defaults, the shortest and the longest search, every non-zero range an edge, and the two
# ends of the sub-pixel term
PARAM_SETS = {
    "default": DEFAULTS,
    "k1": dict(DEFAULTS, searchSteps=1),
    "k16": dict(DEFAULTS, searchSteps=16),
    "all_edges": dict(DEFAULTS, absMin=0, relShift=31),
    "subpix0": dict(DEFAULTS, subpix=0),
    "subpix256": dict(DEFAULTS, subpix=256),
}
# tile edges +- 1 of the kernel's 64 x 32 tile, degenerate frames, and one frame of several tiles each way
SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (63, 31), (64, 32), (65, 33), (130, 70), (322, 190))


def build():
    return build_checker(SRC, LIB, fp=False)


def params_array(params=None):
    p = dict(DEFAULTS, **(params or {}))
    return np.array([p["absMin"], p["relShift"], p["searchSteps"], p["subpix"]], np.uint32)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.aa_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        _REF.aa_ref.restype = None
    return _REF


def checker(img, params=None, row0=0, rows=None, out=None):
    """(rows [row0, row0 + rows) of the anti-aliased (H, W, 4) uint8 frame `img` written into `out` -- a frame of 0xA5 by default --,
    {counter: count over those rows})."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    n = np.zeros(len(COUNTERS), np.uint64)
    p = params_array(params)
    _ref().aa_ref(img.ctypes.data, out.ctypes.data, W, H, row0, rows, p.ctypes.data, n.ctypes.data)
    return out, dict(zip(COUNTERS, (int(v) for v in n)))


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

def slanted_edge(W, H, slope, vertical, polarity, rng=None):
    """Two colours split by a line of slope 1 : slope; vertical: the line runs mostly along y.  polarity swaps the colours."""
    y, x = np.mgrid[0:H, 0:W]
    u, v = (y, x) if vertical else (x, y)
    side = (v * slope) > (u + (min(W, H) * slope) // 3)
    a, b = np.array([230, 220, 40, 255], np.uint8), np.array([20, 30, 160, 128], np.uint8)
    if polarity:
        a, b = b, a
    return np.where(side[..., None], a, b).astype(np.uint8)


def lines(W, H):
    """1-pixel-wide lines: horizontal, vertical and diagonal, bright on dark."""
    img = np.zeros((H, W, 4), np.uint8)
    img[..., :] = (16, 16, 24, 255)
    img[H // 3, :] = (255, 255, 255, 255)
    img[:, W // 3] = (255, 240, 200, 255)
    d = np.arange(min(W, H))
    img[d, d] = (200, 255, 220, 255)
    img[d, (W - 1 - d * 3) % W] = (255, 128, 0, 255)
    return img


def rectangles(W, H, rng, n=24):
    img = np.zeros((H, W, 4), np.uint8)
    img[...] = rng.integers(0, 256, 4, dtype=np.uint8)
    for _ in range(n):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        w, h = int(rng.integers(1, max(2, W // 2))), int(rng.integers(1, max(2, H // 2)))
        img[y0:y0 + h, x0:x0 + w] = rng.integers(0, 256, 4, dtype=np.uint8)
    return img


def varying_alpha(W, H, rng):
    """Piecewise-flat colour, alpha a ramp plus noise: the blend must carry the fourth channel like the others."""
    img = rectangles(W, H, rng, 12)
    y, x = np.mgrid[0:H, 0:W]
    img[..., 3] = ((x * 7 + y * 13) % 256).astype(np.uint8) ^ rng.integers(0, 32, (H, W), dtype=np.uint8)
    return img


def below_threshold(W, H, rng):
    """Luma ranges of at most 77 * 3 + 150 * 3 + 29 * 3 = 768 < absMin = 2048 and < hi >> 3 for hi around 128 * 256: no edge."""
    return (128 + rng.integers(0, 4, (H, W, 4))).astype(np.uint8)


def straight_edge(W, H, vertical):
    """Black left of column W // 2 (above row H // 2), white from it on; opaque."""
    img = np.zeros((H, W, 4), np.uint8)
    img[..., 3] = 255
    if vertical:
        img[:, W // 2:, :3] = 255
    else:
        img[H // 2:, :, :3] = 255
    return img


def oracle_lit_frame(oracle):
    """The 64 x 64 frame the oracle lights from the committed golden planes (three lights, sky fill)."""
    import oracle_lib
    g = dict(np.load(GOLD, allow_pickle=False))
    pcb = oracle_lib.OrPassConstants()
    C.memmove(C.addressof(pcb), g["pass_cb"].tobytes(), C.sizeof(pcb))
    return oracle.deferred_light(pcb, g["g0"], g["g1"], g["g2"], g["depth"], g["blur1_v"], g["shadow"], g["cube"], 3, float(g["pcf_radius"][1]),
                                 sky=True)


_CORPUS = {}


def corpus(oracle):
    """[(name, image)]: every content kind at every one of SIZES, plus a frame below the threshold and the 64 x 64 frame lit by the
    oracle.  Built once and read-only."""
    if "images" in _CORPUS:
        return _CORPUS["images"]
    rng = np.random.default_rng(19)
    out = []
    for W, H in SIZES:
        tag = "%dx%d" % (W, H)
        out.append(("uniform_" + tag, np.full((H, W, 4), 93, np.uint8)))
        out.append(("noise_" + tag, rng.integers(0, 256, (H, W, 4), dtype=np.uint8)))
        out.append(("lines_" + tag, lines(W, H)))
        out.append(("rects_" + tag, rectangles(W, H, rng)))
        out.append(("alpha_" + tag, varying_alpha(W, H, rng)))
        for slope in (1, 5, 20):
            for vertical in (False, True):
                for polarity in (False, True):
                    out.append(("slant%d_%s%d_%s" % (slope, "v" if vertical else "h", polarity, tag), slanted_edge(W, H, slope, vertical, polarity)))
    out.append(("below_threshold_65x33", below_threshold(65, 33, rng)))
    out.append(("oracle_lit_64x64", oracle_lit_frame(oracle)))
    for _, img in out:
        img.setflags(write=False)
    _CORPUS["images"] = out
    return out


_EXPECTED = {}


def expected(name, img, pname):
    """The checker's whole frame and counters for corpus image `name` under PARAM_SETS[pname]; computed once, read-only."""
    key = (name, pname)
    if key not in _EXPECTED:
        out, n = checker(img, PARAM_SETS[pname])
        out.setflags(write=False)
        _EXPECTED[key] = (out, n)
    return _EXPECTED[key]
