"""Builds and loads tests/sharpen_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_sharpen, plain C written from the definition
in include/crychic_hip.h with none of the kernel's code; the frames, the parameter sets and the row ranges the host and the device
tests share."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "sharpen_ref")
SRC, LIB = os.path.join(DIR, "sharpen_ref.c"), os.path.join(DIR, "libsharpenref.so")

MAX_STRENGTH, MAX_LIMIT, DEFAULT_LIMIT = 256, 3584, 3072
# the kernel's geometry (csrc/sharpen_core.hpp): a lane owns 4 pixels of a row, a wavefront 256, a workgroup 1024, and walks 8 rows
QUAD, WAVE_PIXELS, GROUP_PIXELS, STRIP = 4, 256, 1024, 8
# (W, H): below one quad; around the quad; around a wavefront's and a workgroup's width, a few rows high; heights around the strip
TINY = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3))
FRAMES = TINY + ((7, 3), (8, 3), (9, 3),
                 (WAVE_PIXELS - 1, 3), (WAVE_PIXELS, 3), (WAVE_PIXELS + 1, 3), (WAVE_PIXELS + 4, 3),
                 (GROUP_PIXELS - 1, 2), (GROUP_PIXELS, 2), (GROUP_PIXELS + 1, 2), (GROUP_PIXELS + 4, 3),
                 (12, STRIP - 1), (12, STRIP), (12, STRIP + 1), (12, 2 * STRIP + 1), (13, 2 * STRIP + 1))
PARAMS = ((256, DEFAULT_LIMIT), (128, DEFAULT_LIMIT), (1, MAX_LIMIT), (256, MAX_LIMIT), (77, 1000))      # (strength, limit)
MISALIGN = (0, 4, 8, 12)


def build():
    return build_checker(SRC, LIB, fp=False)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.sharpen_ref.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 6
        _REF.sharpen_ref.restype = None
    return _REF


def checker(img, strength=256, limit=DEFAULT_LIMIT, row0=0, rows=None, out=None):
    """Rows [row0, row0 + rows) of the (H, W, 4) uint8 frame `img` sharpened, written into `out` -- a frame of 0xA5 by default."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    assert out.flags.c_contiguous and out.shape == img.shape and 0 <= strength <= MAX_STRENGTH and 0 <= limit <= MAX_LIMIT
    _ref().sharpen_ref(img.ctypes.data, out.ctypes.data, W, H, row0, H - row0 if rows is None else rows, strength, limit)
    return out


# ---- frames: each built once and read-only --------------------------------------------------------------------------------------------

KINDS = ("random", "extreme", "near_flat", "flat", "smooth")
_CORPUS = {}


def frame(W, H, kind="random"):
    """random: every byte uniform; extreme: bytes from {0, 1, 2, 127, 128, 253, 254, 255}; near_flat: a level per channel plus 0 .. 3;
    flat: one colour (alpha still random); smooth: a gradient with a little noise, where the limiter seldom reaches 0."""
    if (W, H, kind) not in _CORPUS:
        rng = np.random.default_rng(1000 * W + 7 * H + KINDS.index(kind))
        if kind == "random":
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        elif kind == "extreme":
            img = np.array([0, 1, 2, 127, 128, 253, 254, 255], np.uint8)[rng.integers(0, 8, (H, W, 4))]
        elif kind == "near_flat":
            img = (rng.integers(0, 253, (1, 1, 4)) + rng.integers(0, 4, (H, W, 4))).astype(np.uint8)
        elif kind == "flat":
            img = np.broadcast_to(rng.integers(0, 256, (1, 1, 4), dtype=np.uint8), (H, W, 4)).copy()
            img[..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
        else:
            y, x = np.mgrid[0:H, 0:W]
            base = np.stack([40 + (3 * x + 2 * y) % 170, 30 + (2 * x + 5 * y) % 190, 60 + (x + y) % 150, x + y], axis=-1)
            img = (base + rng.integers(0, 6, (H, W, 4))).astype(np.uint8)
        img.setflags(write=False)
        _CORPUS[(W, H, kind)] = img
    return _CORPUS[(W, H, kind)]


def row_ranges(H):
    """The whole frame, the inner rows, and one-row ranges at row 0, in the middle and at row H - 1."""
    out = [(0, H)] + ([(1, H - 2)] if H >= 3 else []) + [(0, 1)]
    if H >= 2:
        out += [(H - 1, 1)]
    if H >= 3:
        out += [(H // 2, 1)]
    return out


def stitches(H):
    """Lists of ranges that cover [0, H): single rows; two uneven parts; parts that cut a strip of STRIP rows in two."""
    out = [[(r, 1) for r in range(H)]]
    if H >= 2:
        out.append([(0, H // 3 + 1), (H // 3 + 1, H - H // 3 - 1)])
    if H > STRIP:
        out.append([(0, STRIP - 3), (STRIP - 3, 5), (STRIP + 2, H - STRIP - 2)])
    return [[r for r in ranges if r[1] > 0] for ranges in out]
