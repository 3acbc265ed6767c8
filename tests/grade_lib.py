"""Builds and loads tests/grade_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_grade, plain C written from the definition in
include/crychic_hip.h with none of the kernel's code; the tables, the frames and the .cube writer the host and the device tests
share."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "grade_ref")
SRC, LIB = os.path.join(DIR, "grade_ref.c"), os.path.join(DIR, "libgraderef.so")

MAX_N = 33
SIZES = (2, 3, 16, 17, 32, 33)                                      # both ends, N - 1 dividing 255 (16) and not, the largest even size
FRAMES = ((1, 1), (3, 1), (5, 3), (67, 5), (128, 96))               # (W, H): below one quad, odd widths, more than one workgroup's trip
MISALIGN = (0, 4, 8, 12)


def build():
    return build_checker(SRC, LIB, fp=False)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.grade_ref.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32]
        _REF.grade_ref.restype = None
    return _REF


def checker(img, lut, row0=0, rows=None, out=None):
    """Rows [row0, row0 + rows) of the (H, W, 4) uint8 frame `img` through the (N, N, N, 4) table `lut`, written into `out` -- a frame
    of 0xA5 by default."""
    img = np.ascontiguousarray(img, np.uint8)
    lut = np.ascontiguousarray(lut, np.uint8)
    H, W = img.shape[:2]
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    assert out.flags.c_contiguous and out.shape == img.shape and lut.shape == (lut.shape[0],) * 3 + (4,)
    _ref().grade_ref(img.ctypes.data, out.ctypes.data, W, H, row0, H - row0 if rows is None else rows, lut.ctypes.data, lut.shape[0])
    return out


# ---- tables: (N, N, N, 4) uint8 indexed [blue][green][red] --------------------------------------------------------------------------

def lut_from(fn, N, fourth=255):
    """The table whose entry (i, j, k) is fn(r, g, b) of the rounded bytes r, g, b = round(255 (i, j, k) / (N - 1)), halves up."""
    b = (2 * 255 * np.arange(N) + (N - 1)) // (2 * (N - 1))
    k, j, i = np.meshgrid(b, b, b, indexing="ij")
    lut = np.empty((N, N, N, 4), np.uint8)
    lut[..., 0], lut[..., 1], lut[..., 2] = fn(i, j, k)
    lut[..., 3] = fourth
    return lut


def identity_lut(N):
    return lut_from(lambda r, g, b: (r, g, b), N)


def random_lut(N, rng):
    return rng.integers(0, 256, (N, N, N, 4), dtype=np.uint8)


def write_cube(path, lut, newline="\n", header=None, digits=6):
    """The table as a .cube text file: `header` lines (default: a comment, a title and the size), then N^3 rows of value / 255, red
    fastest.  float_to_unorm8 of a byte / 255 written with six digits is that byte again (the error is below 1e-6 * 255)."""
    N = lut.shape[0]
    lines = list(header) if header is not None else ["# written by tests/grade_lib.py", 'TITLE "test"', "LUT_3D_SIZE %d" % N]
    lines += ["%.*f %.*f %.*f" % (digits, e[0] / 255.0, digits, e[1] / 255.0, digits, e[2] / 255.0) for e in lut.reshape(-1, 4)]
    with open(path, "wb") as f:
        f.write((newline.join(lines) + newline).encode())
    return path


# ---- frames -------------------------------------------------------------------------------------------------------------------------

def all_values_frame():
    """256 x 3: every value of every channel, against a low, a middle and a high value of the other two; alpha counts down."""
    img = np.empty((3, 256, 4), np.uint8)
    v = np.arange(256, dtype=np.uint8)
    img[0] = np.stack([v, np.full(256, 7, np.uint8), np.full(256, 250, np.uint8), 255 - v], axis=1)
    img[1] = np.stack([np.full(256, 128, np.uint8), v, v[::-1], 255 - v], axis=1)
    img[2] = np.stack([v, v, v, 255 - v], axis=1)
    return img


def tie_frame(N):
    """A (3 W, 1)-texel frame on which every pair of fractions ties somewhere, with the third above, below and equal: texels whose
    channel values are drawn from values sharing a fraction under N."""
    n1 = N - 1
    by_f = {}
    for v in range(256):
        p = v * n1
        i = min(p // 255, N - 2)
        by_f.setdefault(p - 255 * i, []).append(v)
    # two different values with one fraction where the size has them (N - 1 sharing a factor with 255), and one value twice
    shared = [vs for vs in by_f.values() if len(vs) >= 2][:12] + [[77, 77], [200, 200]]
    texels = []
    for vs in shared:
        a, b = vs[0], vs[-1]
        for other in (0, 1, 100, 200, 254, 255, a):
            texels += [(a, b, other), (a, other, b), (other, a, b), (a, a, other), (other, b, b), (b, other, a)]
    img = np.array([t + (k & 255,) for k, t in enumerate(texels)], np.uint8).reshape(1, -1, 4)
    return img


_CORPUS = {}


def frame(W, H):
    """A random W x H frame, built once and read-only."""
    if (W, H) not in _CORPUS:
        img = np.random.default_rng(1000 * W + H).integers(0, 256, (H, W, 4), dtype=np.uint8)
        img.reshape(-1, 4)[:: max(1, W * H // 7)] = 255              # white texels: the last cell at its far end
        img.setflags(write=False)
        _CORPUS[(W, H)] = img
    return _CORPUS[(W, H)]


_LUTS = {}


def corpus_lut(N):
    """The random table of size N the host and the device tests share, built once and read-only."""
    if N not in _LUTS:
        lut = random_lut(N, np.random.default_rng(77 + N))
        lut.setflags(write=False)
        _LUTS[N] = lut
    return _LUTS[N]


def row_ranges(H):
    """[0, H), [1, H - 1) and one single row."""
    return [(0, H)] + ([(1, H - 2)] if H >= 3 else []) + [(H // 2, 1)]
