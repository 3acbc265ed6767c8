"""crychic_sharpen on the CPU: the known answers worked by hand that tell misreadings of the definition (include/crychic_hip.h)
apart; the host build of the kernels' bodies (tests/sharpen_host) against the checker (tests/sharpen_ref) and the numpy restatement
(tests/sharpen_restate.py), every byte of every case; the kernel's two division routines against the integer division over every
operand pair the definition can produce; and the refusals, which need no device."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sharpen_host_lib as sh
import sharpen_lib as sl
import sharpen_restate as sr


# ---- known answers: `run(img, strength, limit) -> frame` is the checker here and the device in tests/test_sharpen_gpu.py ---------------

def ring_frame(centre, ring, alpha=9):
    """5 x 5 of `ring` with `centre` in the middle; centre and ring are (R, G, B)."""
    img = np.empty((5, 5, 4), np.uint8)
    img[..., :3] = ring
    img[..., 3] = alpha
    img[2, 2, :3] = centre
    return img


def answers(run):
    # a flat neighbourhood: mn = mx = e, S = 4 e, num = e (16384 - 4 t), den = 4 (4096 - t): out = e at any strength
    flat = np.full((4, 8, 4), 137, np.uint8)
    for strength, limit in ((256, 3584), (256, 3072), (1, 3072)):
        assert np.array_equal(run(flat, strength, limit), flat), "flat 137 does not stay 137"
    # centre 200 in a ring of 100, strength 256, limit 3072:
    #   mn = 100, mx = 200: (100 << 12) / 200 = 2048, ((255 - 200) << 12) / (255 - 100) = 225280 / 155 = 1453 (1453.4): q = 1453
    #   a = min(1453, 3072) = 1453, t = (1453 * 256) >> 8 = 1453, S = 400, num = 16384 * 200 - 1453 * 400 = 2695600,
    #   den = 4 * (4096 - 1453) = 10572, (2695600 + 5286) / 10572 = 255 (255.47)
    got = run(ring_frame((200, 200, 200), (100, 100, 100)), 256, 3072)
    assert tuple(got[2, 2]) == (255, 255, 255, 9), tuple(got[2, 2])
    # the same at strength 128: t = 726, num = 3276800 - 290400 = 2986400, den = 13480, (2986400 + 6740) / 13480 = 222 (222.04)
    got = run(ring_frame((200, 200, 200), (100, 100, 100)), 128, 3072)
    assert tuple(got[2, 2]) == (222, 222, 222, 9), tuple(got[2, 2])
    # the limit binds: centre 128 in a ring of 120: (120 << 12) / 128 = 3840, (127 << 12) / 135 = 3853: q = 3840, a = 3072 = t,
    #   S = 480, num = 2097152 - 1474560 = 622592, den = 4096, (622592 + 2048) / 4096 = 152 (152.5)
    got = run(ring_frame((128, 128, 128), (120, 120, 120)), 256, 3072)
    assert tuple(got[2, 2, :3]) == (152, 152, 152), tuple(got[2, 2])
    # one weight for the three channels, the smallest q: red as above (q = 1453), green flat (q = 4096), blue 250 in a ring of 10:
    #   (10 << 12) / 250 = 163, (5 << 12) / 245 = 83: q = 83 = a = t.  red: num = 3276800 - 33200 = 3243600, den = 16052,
    #   (3243600 + 8026) / 16052 = 202 (202.57); green 50 stays 50; blue: num = 4096000 - 3320 = 4092680, / 16052 = 255 (255.46)
    got = run(ring_frame((200, 50, 250), (100, 50, 10)), 256, 3072)
    assert tuple(got[2, 2, :3]) == (202, 50, 255), tuple(got[2, 2])
    # a 0 or a 255 in the cross of one channel: that channel's q is 0, the pixel is unchanged
    for centre, ring in (((200, 90, 60), (100, 0, 30)), ((200, 90, 60), (100, 255, 30)), ((0, 90, 60), (100, 20, 30)), ((255, 90, 60), (100, 20, 30))):
        img = ring_frame(centre, ring)
        assert tuple(run(img, 256, 3584)[2, 2]) == tuple(img[2, 2]), (centre, ring)
    # strength 0 and limit 0 are the identity; alpha never changes
    noise = sl.frame(13, 2 * sl.STRIP + 1)
    assert np.array_equal(run(noise, 0, 3072), noise) and np.array_equal(run(noise, 256, 0), noise), "strength 0 or limit 0 changes a byte"
    smooth = sl.frame(13, 2 * sl.STRIP + 1, "smooth")
    got = run(smooth, 256, 3072)
    assert np.array_equal(got[..., 3], smooth[..., 3]), "alpha does not survive"
    assert (got[..., :3] != smooth[..., :3]).mean() > 0.5, "the smooth frame is hardly sharpened: the cases behind it show little"


def test_known_answers_checker():
    answers(lambda img, s, l: sl.checker(img, s, l))


def test_known_answers_restatement():
    answers(lambda img, s, l: sr.apply(img, s, l))


def _cases():
    """(name, frame, strength, limit)."""
    out = []
    for kind in sl.KINDS:
        for W, H in ((13, 2 * sl.STRIP + 1), (8, 3), (1, 5), (5, 1)):
            for strength, limit in sl.PARAMS:
                out.append(("%s %dx%d s=%d l=%d" % (kind, W, H, strength, limit), sl.frame(W, H, kind), strength, limit))
    for strength, limit in ((0, 3072), (256, 0), (1, 3072), (128, 3584), (256, 3584)):
        out.append(("random 67x9 s=%d l=%d" % (strength, limit), sl.frame(67, 9), strength, limit))
    return out


def test_restatement_equals_checker():
    """And the restatement asserts on each case that no numerator is below 0 and no output above 255."""
    for name, img, strength, limit in _cases():
        assert np.array_equal(sr.apply(img, strength, limit), sl.checker(img, strength, limit)), name


def _ranged_cases():
    """The cases, and the smooth frame in row ranges: only there can a clamp to the rows show."""
    out = [(name, img, s, l, 0, img.shape[0]) for name, img, s, l in _cases()]
    img = sl.frame(13, 2 * sl.STRIP + 1, "smooth")
    for row0, rows in sl.row_ranges(img.shape[0]):
        out.append(("smooth rows %d+%d" % (row0, rows), img, 256, 3072, row0, rows))
    return out


@pytest.mark.parametrize("mutation", sr.MUTATIONS)
def test_restatement_bites(mutation):
    """One misreading of the header made on purpose in the restatement: a comparison with the checker must fail on the cases above."""
    fails = []
    for name, img, strength, limit, row0, rows in _ranged_cases():
        if not np.array_equal(sr.apply(img, strength, limit, row0, rows, mutation), sl.checker(img, strength, limit, row0, rows)[row0:row0 + rows]):
            fails.append(name)
    print("%s: %d of %d comparisons fail, the first: %s" % (mutation, len(fails), len(_ranged_cases()), fails[:1]))
    assert fails, "the cases cannot tell %s from the header's text" % mutation


# ---- the CPU tier: the host build of the kernels' bodies --------------------------------------------------------------------------------

def run_host(img, strength=256, limit=3072, misalign=0, out_misalign=None, ranges=None):
    """The bodies over guarded planes `misalign` / `out_misalign` bytes past a 64-byte boundary: the frame, guards and input checked."""
    raw_in, src = sl.guarded(img.shape, np.uint8, misalign=misalign)
    src[...] = img
    raw_out, out = sl.guarded(img.shape, np.uint8, misalign=misalign if out_misalign is None else out_misalign)
    stats = {}
    for row0, rows in ranges or [(0, img.shape[0])]:
        stats = sh.sharpen(src, out, strength, limit, row0, rows)
    assert sl.guards_intact(raw_in, src) and sl.guards_intact(raw_out, out), "a guard byte changed"
    assert np.array_equal(src, img), "the input changed"
    return out.copy(), stats


def test_host_known_answers():
    answers(lambda img, s, l: run_host(img, s, l)[0])
    answers(lambda img, s, l: run_host(img, s, l, misalign=12)[0])


@pytest.mark.parametrize("kind", sl.KINDS)
def test_host_equals_checker_equals_restatement(kind):
    for W, H in sl.FRAMES:
        img = sl.frame(W, H, kind)
        for strength, limit in sl.PARAMS if W * H <= 600 else sl.PARAMS[:2]:
            ref = sl.checker(img, strength, limit)
            if W * H <= 600:
                assert np.array_equal(sr.apply(img, strength, limit), ref), (W, H, strength, limit)
            for misalign in sl.MISALIGN:
                got, stats = run_host(img, strength, limit, misalign=misalign)
                assert np.array_equal(got, ref), "%dx%d, %d bytes past a 16-byte boundary, strength %d, limit %d: %d bytes differ" % (
                    W, H, misalign, strength, limit, int((got != ref).sum()))
                assert stats["wide_launches"] == (1 if W % 4 == 0 and misalign == 0 else 0)
            got, stats = run_host(img, strength, limit, misalign=0, out_misalign=8)
            assert np.array_equal(got, ref) and stats["wide_launches"] == 0, "%dx%d, planes aligned differently" % (W, H)


@pytest.mark.parametrize("W,H", [(12, 2 * sl.STRIP + 1), (13, 2 * sl.STRIP + 1), (sl.WAVE_PIXELS + 4, 3), (5, 1), (1, 5)])
def test_host_row_ranges(W, H):
    """A range writes its rows and no other byte, reads the rows beside it from the frame, and ranges stitch to the whole frame."""
    img = sl.frame(W, H, "smooth")
    ref = sl.checker(img)
    for row0, rows in sl.row_ranges(H):
        for misalign in (0, 4):
            got, _ = run_host(img, misalign=misalign, ranges=[(row0, rows)])
            want = np.full_like(ref, sl.GUARD)
            want[row0:row0 + rows] = ref[row0:row0 + rows]
            assert np.array_equal(got, want), (W, H, row0, rows, misalign)
    assert (run_host(img, ranges=[(0, 0)])[0] == sl.GUARD).all(), "rows == 0 wrote"
    for ranges in sl.stitches(H):
        assert np.array_equal(run_host(img, ranges=ranges)[0], ref), ranges


# ---- the division routines, exhaustively -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ulps", (0, -1, 1))
def test_q12_is_the_floor(ulps):
    """floor(4096 n / d) over every n <= d <= 255 -- the pairs mn / mx and (255 - mx) / (255 - mn) of mn <= mx <= 255 --, with the
    host's reciprocal and with one a unit in the last place either way, where the device's may lie."""
    assert sh.q12_mismatches(ulps) == 0


@pytest.mark.parametrize("ulps", (0, -1, 1))
def test_div_is_the_floor(ulps):
    """(num + den / 2) / den over every t <= 3584 and every num < 2^22, the reciprocal as above."""
    workers = max(1, min(16, os.cpu_count() or 1))
    cuts = np.linspace(0, sl.MAX_LIMIT + 1, 4 * workers + 1).astype(int)
    with ThreadPoolExecutor(workers) as pool:
        bad = sum(pool.map(lambda k: sh.div_mismatches(int(cuts[k]), int(cuts[k + 1]), ulps), range(len(cuts) - 1)))
    assert bad == 0


def test_the_division_counters_can_count():
    """A reciprocal sixteen units off must show in both: a counter that cannot fail proves nothing."""
    assert sh.q12_mismatches(-16) > 0 and sh.q12_mismatches(16) > 0
    assert sh.div_mismatches(0, 8, 16) > 0 and sh.div_mismatches(3577, 3585, -16) > 0


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_need_no_device(built_lib):
    f, err = built_lib.lib.crychic_sharpen, built_lib.lib.crychic_last_error
    P = built_lib.SharpenParams
    buf = np.zeros(64 * 32 * 4 * 2 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    a, b = C.c_void_p(base), C.c_void_p(base + 64 * 32 * 4)
    W, H = 64, 32

    def params(strength=128, limit=3072, r0=0, r1=0):
        p = P()
        p.strength, p.limit, p.reserved[0], p.reserved[1] = strength, limit, r0, r1
        return C.byref(p)
    assert f(None, a, b, W, H, 0, H, params(strength=257), None) == -1 and "strength 257 outside 0 .. 256" in err().decode()
    assert f(None, a, b, W, H, 0, H, params(limit=3585), None) == -1 and "limit 3585 outside 0 .. 3584" in err().decode()
    assert f(None, a, b, W, H, 0, H, params(r0=1), None) == -1 and "reserved" in err().decode()
    assert f(None, a, b, W, H, 0, H, params(r1=1), None) == -1 and "reserved" in err().decode()
    assert f(None, None, b, W, H, 0, H, None, None) == -1 and "null argument" in err().decode()
    assert f(None, a, None, W, H, 0, H, None, None) == -1 and "null argument" in err().decode()
    assert f(None, a, b, W, H, 1, H, None, None) == -1 and "rows" in err().decode()
    assert f(None, a, b, W, H, H + 1, 0, None, None) == -1 and "rows" in err().decode()
    assert f(None, a, b, 0, H, 0, 0, None, None) == -1 and f(None, a, b, W, 0, 0, 0, None, None) == -1
    assert f(None, a, a, W, H, 0, H, None, None) == -1 and "overlap" in err().decode()             # in place: the pass reads neighbours
    assert f(None, a, C.c_void_p(base + 16), W, H, 0, H, None, None) == -1 and "overlap" in err().decode()
    assert f(None, C.c_void_p(base + 64 * 32 * 4 - 4), a, W, H, 0, H, None, None) == -1 and "overlap" in err().decode()
    assert f(None, a, C.c_void_p(b.value + 2), W, H, 0, H, None, None) == -1 and "aligned" in err().decode()
    assert f(None, C.c_void_p(base + 1), b, W, H, 0, H, None, None) == -1 and "aligned" in err().decode()
    assert f(None, a, b, 1 << 15, (1 << 13) + 1, 0, 1, None, None) == -4 and "2^28" in err().decode()
    # everything in order but the context: any size, any 4-byte alignment, the defaults and both ends of the ranges
    for args in ((W, H, 0, H, None), (W, H, 0, H, params(0, 0)), (W, H, H - 1, 1, params(256, 3584)), (63, 31, 30, 1, None), (1, 1, 0, 1, None)):
        assert f(None, a, C.c_void_p(b.value + 4), *args, None) == -1 and "null context" in err().decode(), args
    assert built_lib.lib.crychic_sharpen_default_params(None) == -1
    d = P.default()
    assert d.limit == sl.DEFAULT_LIMIT and 0 <= d.strength <= 256 and d.strength % 32 == 0 and list(d.reserved) == [0, 0]
    assert C.sizeof(P) == 16
