"""crychic_taa_upscale on the CPU tier: the kernel body (csrc/taa_upscale_core.hpp, built for the host with the workgroup and lane walk
emulated) against the checker (tests/taa_upscale_ref, plain C from the definition in include/crychic_hip.h), byte for byte in both
outputs on the whole corpus, behind guard bytes and on misaligned planes; what the corpus must reach; the definition's known answers,
the ratio-1 case against crychic_taa's checker among them; the position's 32-bit path against exact integers; row ranges; convergence
on the analytic still scene; and the refusals of the real library, which need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import taa_lib as ta
import taa_upscale_host_lib as host
import taa_upscale_lib as tu


@pytest.fixture(scope="module")
def cases(built_lib):
    return tu.corpus()


def run_host(case, row0=0, rows=None, misalign=0):
    """The kernel body on guarded copies of the case's planes, `misalign` bytes past a 64-byte boundary (8 for the history planes' own
    alignment): (out, history_out); asserts the guard bytes around every plane and that no input changed."""
    Ho, Wo = case.Ho, case.Wo
    sraw, src = tu.guarded(case.img.shape, misalign=misalign)
    draw, depth = tu.guarded(case.depth.shape, np.uint32, misalign=misalign)
    oraw, out = tu.guarded((Ho, Wo, 4), misalign=misalign)
    horaw, hout = tu.guarded((Ho, Wo, 4), np.uint16, misalign=misalign & 8)
    src[...] = case.img
    depth[...] = case.depth
    hist, hiraw = None, None
    if case.hist is not None:
        hiraw, hist = tu.guarded((Ho, Wo, 4), np.uint16, misalign=misalign & 8)
        hist[...] = case.hist
    c = tu.Case(case.name, case.ivp, case.cur, case.prev, case.jitter, depth, src, (Wo, Ho), hist, case.blend, case.flags)
    c.img, c.depth, c.hist = src, depth, hist              # the guarded planes themselves, not copies
    host.taa_upscale(c, row0, rows, out, hout)
    for raw, view in ((sraw, src), (draw, depth), (oraw, out), (horaw, hout)) + (() if hist is None else ((hiraw, hist),)):
        assert tu.guards_intact(raw, view), "guard bytes changed"
    assert np.array_equal(src, case.img) and np.array_equal(depth, case.depth) and (hist is None or np.array_equal(hist, case.hist)), "an input plane changed"
    return out.copy(), hout.copy()


def test_host_body_equals_checker(cases):
    for n, case in enumerate(cases):
        ref_out, ref_hist, _ = tu.expected(case)
        for misalign in ((0, 4, 12) if n % 8 == 0 or "vote" in case.name else ((0, 4, 12)[n % 3],)):
            out, hist = run_host(case, misalign=misalign)
            assert np.array_equal(out, ref_out), "%s (+%d): %d bytes of out differ" % (case.name, misalign, int((out != ref_out).sum()))
            assert np.array_equal(hist, ref_hist), "%s (+%d): %d words of history_out differ" % (case.name, misalign, int((hist != ref_hist).sum()))
    assert len(cases) >= len(tu.SHAPES) * len(tu.jitters()) * len(tu.MOTIONS)


def test_the_corpus_reaches_what_it_must(cases):
    """With the checker alone: every shape, jitter and motion is there, no branch is empty, every weight from 0 to the blend occurs,
    and every vote of the kernel meets a wavefront with one lane on either side."""
    assert {(c.Wi, c.Hi, c.Wo, c.Ho) for c in cases} >= set(tu.SHAPES)
    assert {c.jitter for c in cases} >= set(tu.jitters())
    assert {c.blend for c in cases} >= {1, 102, 256} and {c.flags for c in cases} >= {0, tu.RESET, tu.NO_CLAMP}
    n = dict(history=0, no_history=0, fx_zero=0, fx_nonzero=0, fy_zero=0, fy_nonzero=0, clamped=0, unclamped=0)
    seen = set()
    for c in cases:
        b = tu.expected(c)[2]
        h = (b & tu.B_HISTORY) != 0
        n["history"] += int(h.sum())
        n["no_history"] += int((~h).sum())
        n["fx_nonzero"] += int(((b & tu.B_FX) != 0).sum())
        n["fx_zero"] += int((h & ((b & tu.B_FX) == 0)).sum())
        n["fy_nonzero"] += int(((b & tu.B_FY) != 0).sum())
        n["fy_zero"] += int((h & ((b & tu.B_FY) == 0)).sum())
        if not c.flags & tu.NO_CLAMP:
            n["clamped"] += int(((b & tu.B_CLAMPED) != 0).sum())
            n["unclamped"] += int((h & ((b & tu.B_CLAMPED) == 0)).sum())
        w = tu.weights(c)
        assert np.array_equal(w, tu.np_current(c)[2]), c.name
        seen |= {(c.blend, int(v)) for v in np.unique(w)}
    print("pixels per branch:", n)
    assert all(v > 0 for v in n.values()), n
    assert {(256, 256), (256, 0), (102, 102), (102, 0), (1, 0), (1, 1)} <= seen, "a sample on the centre and one a pixel away, per blend"
    by_name = {c.name: c for c in cases}
    for axis, bit in (("hist", tu.B_HISTORY), ("fx", tu.B_FX), ("fy", tu.B_FY)):
        both = np.concatenate([tu.wave_counts(tu.expected(by_name["vote_%s_%s" % (axis, k)])[2], bit) for k in ("one_lane", "all_but_one")])
        assert (both == 1).any() and (both == 63).any(), (axis, both)


def test_known_answers(built_lib):
    tu.answers(lambda c: tu.checker(c)[:2])
    tu.answers(lambda c: run_host(c))
    tu.answers(lambda c: run_host(c, misalign=12))


def test_position_paths_against_exact_integers(built_lib):
    """Step 1 with Python's integers against the body's 32-bit path (sizes whose product is below 2^24) and its 64-bit path (any size up
    to 2^22 a side), at both ends of the row and at random pixels."""
    rng = np.random.default_rng(1)
    for Ni, No, narrow in ((2560, 3840, True), (1440, 2160, True), (4095, 4096, True), (1, 4, True), (1 << 20, 1 << 22, False), (1 << 22, 1 << 22, False),
                           ((1 << 22) - 1, (1 << 22), False), (4097, 4096 * 3, False), (2560, 3840, False)):
        assert (No * Ni * 256 <= 0xFFFFFFFF) or not narrow
        for o in [0, 1, No // 2, No - 2, No - 1] + [int(v) for v in rng.integers(0, No, 64)]:
            for J in (-128, 0, 37, 128):
                assert host.position(o, Ni, No, J, narrow) == ((2 * o + 1) * Ni * 256) // (2 * No) + J - 128, (Ni, No, o, J)


def test_division_by_a_host_divisor_is_exact(built_lib):
    """tu_div against Python's integers: small and large divisors, numerators at the multiples of the divisor, one either side of them,
    at both ends of 32 bits and at random."""
    rng = np.random.default_rng(2)
    for d in [1, 2, 3, 7, 255, 256, 1440, 2160, 2560, 3840, 65535, 65536, (1 << 22) - 1, 1 << 22, (1 << 31) - 1, 1 << 31, (1 << 32) - 1] + \
            [int(v) for v in rng.integers(1, 1 << 32, 40)]:
        ns = {0, 1, d - 1, d, d + 1, (1 << 32) - 1, (1 << 32) - 2, ((1 << 32) - 1) // d * d, max(((1 << 32) - 1) // d * d - 1, 0)}
        ns |= {int(k) * d + e for k in rng.integers(0, (1 << 32) // d + 1, 8) for e in (-1, 0, 1)} | {int(v) for v in rng.integers(0, 1 << 32, 16)}
        for n in ns:
            if 0 <= n < 1 << 32:
                assert host.div(n, d) == n // d, (n, d)


def tall_case(motion):
    rng = np.random.default_rng(191)
    Wi, Hi, Wo, Ho = 30, 100, 45, 190
    img = rng.integers(0, 256, (Hi, Wi, 4), dtype=np.uint8)
    ivp, cur, prev = ta.motion_matrices(motion, Wi, Hi)
    return tu.Case("tall_" + motion, ivp, cur, prev, (0.25, -0.375), ta.make_depth("random", Wi, Hi, rng), img, (Wo, Ho),
                   rng.integers(0, 1 << 16, (Ho, Wo, 4), dtype=np.uint16))


SPLITS = [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 189, 190)]


@pytest.mark.parametrize("split", SPLITS)
def test_row_ranges_stitch_to_the_whole_frame(built_lib, split):
    for motion in ("dolly", "subpixel_pan"):
        case = tall_case(motion)
        whole_out, whole_hist, _ = tu.checker(case)
        s_out, s_hist = np.full_like(whole_out, tu.GUARD), np.full_like(whole_hist, tu.GUARD * 257)
        for row0, end in zip(split[:-1], split[1:]):
            out, hist = run_host(case, row0=row0, rows=end - row0)
            ref_out, ref_hist, _ = tu.checker(case, row0=row0, rows=end - row0)
            assert np.array_equal(out, ref_out) and np.array_equal(hist, ref_hist), (motion, row0, end)
            for plane, guard in ((out, tu.GUARD), (hist, tu.GUARD * 257)):
                assert (plane[:row0] == guard).all() and (plane[end:] == guard).all(), "rows outside the range were written"
            s_out[row0:end], s_hist[row0:end] = out[row0:end], hist[row0:end]
        assert np.array_equal(s_out, whole_out) and np.array_equal(s_hist, whole_hist), motion
    out, hist = run_host(case, row0=190, rows=0)
    assert (out == tu.GUARD).all() and (hist == tu.GUARD * 257).all()


def test_default_params(built_lib):
    p = built_lib.TaaUpscaleParams()
    assert C.sizeof(p) == 32 and built_lib.lib.crychic_taa_upscale_default_params(C.byref(p)) == 0
    assert (p.blend, p.flags, tuple(p.reserved)) == (tu.DEFAULT_BLEND, 0, (0,) * 6)
    assert built_lib.lib.crychic_taa_upscale_default_params(None) == -1
    q = built_lib.TaaUpscaleParams.default(blend=64, flags=built_lib.TAA_NO_CLAMP)
    assert (q.blend, q.flags) == (64, 2)


# ---- convergence ----------------------------------------------------------------------------------------------------------------------

def convergence(fn):
    """(accumulated, bilinear, negated): the mean absolute RGB errors, against 8 x 8 supersamples per display pixel, of 16 jittered
    160 x 90 frames of the analytic scene accumulated at 240 x 135 by fn, of one unjittered frame upsampled bilinearly, and of the same
    accumulation with the pass told the opposite jitter."""
    Wi, Hi, Wo, Ho = 160, 90, 240, 135
    truth = tu.analytic_truth(Wo, Ho)
    acc = tu.mean_abs_error(tu.still_sequence(fn, Wi, Hi, Wo, Ho, 16), truth)
    neg = tu.mean_abs_error(tu.still_sequence(fn, Wi, Hi, Wo, Ho, 16, negate=True), truth)
    return acc, tu.mean_abs_error(tu.bilinear_frame(Wi, Hi, Wo, Ho), truth), neg


def test_convergence_on_the_analytic_scene(built_lib):
    """The accumulated frame is closer to the supersampled truth than a single frame upsampled bilinearly, and closer than the same
    run with the jitter negated in the pass call: the sign of step 1 is the header's.  Measured, analytic scene of tests/taa_upscale_lib.py:
    21.15 accumulated, 34.20 bilinear, 45.14 negated (profiles/taa_upscale_quality.txt)."""
    acc, bil, neg = convergence(lambda c: tu.checker(c)[:2])
    print("mean absolute error: %.2f accumulated, %.2f bilinear, %.2f with the jitter negated" % (acc, bil, neg))
    assert acc < bil and acc < neg


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, P = built_lib.lib, built_lib.TaaUpscaleParams
    Wi, Hi, Wo, Ho = 64, 32, 96, 48
    a, b, d, hi, ho = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000           # never dereferenced
    ib, ob, hb = Wi * Hi * 4, Wo * Ho * 4, Wo * Ho * 8
    good = built_lib.PassConstants()
    good.InvViewProj[:] = list(ta.IDENTITY)
    eye = (C.c_float * 16)(*ta.IDENTITY)

    def mat(k, v):
        m = (C.c_float * 16)(*ta.IDENTITY)
        m[k] = v
        return m

    def call(cb=good, cur=eye, prev=eye, jx=0.25, jy=-0.5, depth=d, src=a, Wi=Wi, Hi=Hi, hin=hi, hout=ho, dst=b, Wo=Wo, Ho=Ho, row0=0, rows=Ho, params=None):
        rc = lib.crychic_taa_upscale(None, None if cb is None else C.byref(cb), cur, prev, jx, jy, depth, src, Wi, Hi, hin, hout, dst, Wo, Ho, row0, rows,
                                     None if params is None else C.byref(params), None)
        return rc, lib.crychic_last_error().decode()

    ok = (-1, "null context")
    assert call() == ok
    assert call(dst=a + ib) == ok and call(hout=hi + hb) == ok and call(hin=a + ib, dst=a + ib + hb) == ok, "adjacent planes do not overlap"
    assert call(row0=Ho, rows=0) == ok and call(Wi=1, Hi=1, Wo=4, Ho=4, rows=4) == ok and call(Wi=1, Hi=1, Wo=1, Ho=1, rows=1) == ok
    assert call(Wo=Wi, Ho=4 * Hi, rows=1) == ok and call(Wo=4 * Wi, Ho=Hi, rows=Hi) == ok, "the two ratios are independent"
    assert call(params=P.default(blend=1)) == ok and call(params=P.default(blend=256, flags=3)) == ok
    assert call(jx=0.5, jy=0.5) == ok and call(jx=-0.5, jy=0.0) == ok
    assert call(hin=None, params=P.default(flags=tu.RESET)) == ok, "history_in may be NULL with RESET"
    assert call(hin=hi + 8, hout=ho + 8, src=a + 4, dst=b + 4, depth=d + 12) == ok
    bad_res = P.default()
    bad_res.reserved[5] = 1
    bad_cb = built_lib.PassConstants.from_buffer_copy(good)
    bad_cb.InvViewProj[7] = math.inf
    for kw, word in ((dict(cb=None), "null argument"), (dict(cur=None), "null argument"), (dict(prev=None), "null argument"),
                     (dict(depth=None), "null argument"), (dict(src=None), "null argument"), (dict(hin=None), "null argument"),
                     (dict(hout=None), "null argument"), (dict(dst=None), "null argument"),
                     (dict(hout=None, params=P.default(flags=tu.RESET)), "null argument"),
                     (dict(src=a + 2), "4-byte aligned"), (dict(dst=b + 1), "4-byte aligned"), (dict(depth=d + 2), "4-byte aligned"),
                     (dict(hin=hi + 4), "8-byte aligned"), (dict(hout=ho + 4), "8-byte aligned"),
                     (dict(Wi=0), "non-zero"), (dict(Hi=0), "non-zero"), (dict(Wo=0), "non-zero"), (dict(Ho=0, rows=0), "non-zero"),
                     (dict(Wo=Wi - 1), "ratio"), (dict(Wo=4 * Wi + 1), "ratio"), (dict(Ho=Hi - 1, rows=1), "ratio"), (dict(Ho=4 * Hi + 1), "ratio"),
                     (dict(Wi=0x80000000, Wo=2, Hi=1, Ho=1, rows=1), "ratio"),
                     (dict(row0=Ho + 1, rows=0), "outside the 48-row frame"), (dict(row0=1, rows=Ho), "outside the 48-row frame"),
                     (dict(row0=0xFFFFFFFF, rows=2), "outside the 48-row frame"),
                     (dict(jx=math.nan), "jitter"), (dict(jy=math.inf), "jitter"), (dict(jx=0.5000001), "jitter"), (dict(jy=-0.75), "jitter"),
                     (dict(cb=bad_cb), "not finite"), (dict(cur=mat(0, math.nan)), "not finite"), (dict(prev=mat(15, -math.inf)), "not finite"),
                     (dict(params=P.default(blend=0)), "blend"), (dict(params=P.default(blend=257)), "blend"),
                     (dict(params=P.default(flags=4)), "flags"), (dict(params=P.default(flags=0x80000001)), "flags"), (dict(params=bad_res), "reserved"),
                     (dict(dst=a), "overlaps an input"), (dict(dst=a + ib - 4), "overlaps an input"), (dict(src=b + ob - 4), "overlaps an input"),
                     (dict(dst=d + 4), "overlaps an input"), (dict(depth=b + ob - 4), "overlaps an input"),
                     (dict(hout=hi), "history planes overlap"), (dict(hout=hi + hb - 8), "history planes overlap"),
                     (dict(hin=ho + hb - 8), "history planes overlap"),
                     (dict(hout=hi, params=P.default(flags=tu.RESET)), "history planes overlap"),
                     (dict(hin=a + ib - 8), "overlaps a frame plane"), (dict(hout=b + 8), "overlaps a frame plane"), (dict(hout=d + ib - 8), "overlaps a frame plane"),
                     (dict(hin=b - hb + 8), "overlaps a frame plane"), (dict(hout=a, params=P.default(flags=tu.RESET), hin=None), "overlaps a frame plane")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = call(Wi=1 << 15, Hi=(1 << 13) + 1, Wo=1 << 15, Ho=(1 << 13) + 1, rows=1)
    assert rc == -4 and "exceeds" in msg
    rc, msg = call(Wi=(1 << 22) + 1, Hi=1, Wo=(1 << 22) + 1, Ho=1, rows=1)
    assert rc == -4 and "2^22" in msg
    assert call(Wi=1 << 20, Hi=1, Wo=1 << 22, Ho=1, rows=1) == ok
