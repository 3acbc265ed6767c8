"""crychic_taa on the CPU tier: the kernel body (csrc/taa_core.hpp, built for the host with the workgroup and lane walk emulated)
against the checker (tests/taa_ref, plain C from the definition in include/crychic_hip.h), byte for byte in both outputs on the whole
corpus, behind guard bytes and on misaligned planes; what the corpus must reach, with the share of pixels in each branch; the
definition's known answers; row ranges; the jitter sequence and the jittered constant builders; the jittered ray-caster; convergence
on the still scene against a supersampled frame; and the refusals of the real library, which need no device."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import taa_host_lib as host
import taa_lib as ta


@pytest.fixture(scope="module")
def cases(built_lib):
    return ta.corpus()


def run_host(case, row0=0, rows=None, misalign=0):
    """The kernel body on guarded copies of the case's planes, `misalign` bytes past a 16-byte boundary (8 for the history planes' own
    alignment): (out, history_out); asserts the guard bytes around every plane and that no input changed."""
    H, W = case.H, case.W
    sraw, src = ta.guarded(case.img.shape, misalign=misalign)
    draw, depth = ta.guarded(case.depth.shape, np.uint32, misalign=misalign)
    oraw, out = ta.guarded(case.img.shape, misalign=misalign)
    horaw, hout = ta.guarded((H, W, 4), np.uint16, misalign=misalign & 8)
    src[...] = case.img
    depth[...] = case.depth
    hist, hiraw = None, None
    if case.hist is not None:
        hiraw, hist = ta.guarded((H, W, 4), np.uint16, misalign=misalign & 8)
        hist[...] = case.hist
    c = ta.Case(case.name, case.ivp, case.cur, case.prev, depth, src, hist, case.blend, case.flags)
    c.img, c.depth, c.hist = src, depth, hist              # the guarded planes themselves, not copies
    host.taa(c, row0, rows, out, hout)
    for raw, view in ((sraw, src), (draw, depth), (oraw, out), (horaw, hout)) + (() if hist is None else ((hiraw, hist),)):
        assert ta.guards_intact(raw, view), "guard bytes changed"
    assert np.array_equal(src, case.img) and np.array_equal(depth, case.depth) and (hist is None or np.array_equal(hist, case.hist)), "an input plane changed"
    return out.copy(), hout.copy()


def test_the_kernel_tile_is_what_the_sizes_assume(built_lib):
    assert host.tile() == (ta.TILE_W, ta.TILE_H)
    for d in (-1, 0, 1):
        assert any(W == ta.TILE_W + d for W, _ in ta.SIZES) and any(H == ta.TILE_H + d for _, H in ta.SIZES)


def test_host_body_equals_checker(cases):
    for case in cases:
        ref_out, ref_hist, _ = ta.expected(case)
        for misalign in (0, 4, 12):
            out, hist = run_host(case, misalign=misalign)
            assert np.array_equal(out, ref_out), "%s (+%d): %d bytes of out differ" % (case.name, misalign, int((out != ref_out).sum()))
            assert np.array_equal(hist, ref_hist), "%s (+%d): %d words of history_out differ" % (case.name, misalign, int((hist != ref_hist).sum()))
    assert len(cases) >= len(ta.SIZES) * len(ta.MOTIONS)


def test_the_corpus_reaches_what_it_must(cases):
    """With the checker alone: every size and motion is there, no branch is empty, history values above 65280 occur, and every vote of
    the kernel meets a wavefront with one lane on either side.  Prints the share of pixels in each branch."""
    assert {(c.W, c.H) for c in cases} >= set(ta.SIZES)
    assert all(any(m in c.name for c in cases if (c.W, c.H) == s) for m in ta.MOTIONS for s in ta.SIZES)
    assert any(c.hist is not None and (c.hist > 65280).any() for c in cases)
    assert {c.blend for c in cases} >= {1, 26, 128, 255, 256} and {c.flags for c in cases} >= {0, ta.RESET, ta.NO_CLAMP}
    n = dict(pixels=0, history=0, no_history=0, fx_zero=0, fx_nonzero=0, fy_zero=0, fy_nonzero=0, clamped=0, unclamped=0)
    waves = dict(no_history=0, some_history=0, right_taps_dropped=0, right_taps_read=0, lower_taps_dropped=0, lower_taps_read=0)
    for c in cases:
        b = ta.expected(c)[2]
        h = (b & ta.B_HISTORY) != 0
        n["pixels"] += b.size
        n["history"] += int(h.sum())
        n["no_history"] += int((~h).sum())
        n["fx_nonzero"] += int(((b & ta.B_FX) != 0).sum())
        n["fx_zero"] += int((h & ((b & ta.B_FX) == 0)).sum())
        n["fy_nonzero"] += int(((b & ta.B_FY) != 0).sum())
        n["fy_zero"] += int((h & ((b & ta.B_FY) == 0)).sum())
        if not c.flags & ta.NO_CLAMP:
            n["clamped"] += int(((b & ta.B_CLAMPED) != 0).sum())
            n["unclamped"] += int((h & ((b & ta.B_CLAMPED) == 0)).sum())
        hc, fxc, fyc = (ta.wave_counts(b, bit) for bit in (ta.B_HISTORY, ta.B_FX, ta.B_FY))
        waves["no_history"] += int((hc == 0).sum())
        waves["some_history"] += int((hc > 0).sum())
        waves["right_taps_dropped"] += int(((hc > 0) & (fxc == 0)).sum())
        waves["right_taps_read"] += int((fxc > 0).sum())
        waves["lower_taps_dropped"] += int(((hc > 0) & (fyc == 0)).sum())
        waves["lower_taps_read"] += int((fyc > 0).sum())
    print("pixels per branch:", {k: "%d (%.1f %%)" % (v, 100.0 * v / n["pixels"]) for k, v in n.items()})
    print("whole wavefronts per vote:", waves)
    assert all(v > 0 for v in n.values()), n
    assert all(v > 0 for v in waves.values()), waves
    # each vote: a wavefront with exactly one lane on one side, and one with exactly one lane on the other
    by_name = {c.name: c for c in cases}
    for axis, bit in (("hist", ta.B_HISTORY), ("fx", ta.B_FX), ("fy", ta.B_FY)):
        for name in ("vote_%s_one_lane" % axis, "vote_%s_all_but_one" % axis):
            counts = ta.wave_counts(ta.expected(by_name[name])[2], bit)
            assert (counts == 1).any() or (counts == 63).any(), (name, counts)
        both = np.concatenate([ta.wave_counts(ta.expected(by_name["vote_%s_%s" % (axis, k)])[2], bit) for k in ("one_lane", "all_but_one")])
        assert (both == 1).any() and (both == 63).any(), (axis, both)


def answers(fn):
    """The definition's known answers for fn(case) -> (out, history_out)."""
    rng = np.random.default_rng(5)
    W, H = 70, 38
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    depth = ta.make_depth("random", W, H, rng)
    noise = ta.make_history("random", img, rng)
    img256 = img.astype(np.uint16) * 256
    ivp, cur, prev = ta.motion_matrices("dolly", W, H)
    # RESET: out == in, history_out == 256 in
    for hist in (noise, None):
        out, hout = fn(ta.Case("reset", ivp, cur, prev, depth, img, hist, flags=ta.RESET))
        assert np.array_equal(out, img) and np.array_equal(hout, img256)
    # blend == 256: out == in whatever the history
    for flags in (0, ta.NO_CLAMP):
        out, hout = fn(ta.Case("blend256", ivp, cur, prev, depth, img, noise, blend=256, flags=flags))
        assert np.array_equal(out, img) and np.array_equal(hout, img256)
    # identical matrices over history_in == 256 in: a fixed point
    out, hout = fn(ta.Case("fixed_point", ivp, cur, cur, depth, img, img256))
    assert np.array_equal(out, img) and np.array_equal(hout, img256)
    # a constant frame over a constant history, identical matrices: the closed form without the clamp, the frame itself with it
    Cc, Hc = np.array([200, 17, 96, 33], np.uint8), np.array([1234, 65535, 24576, 999], np.uint16)
    flat, flat_h = np.broadcast_to(Cc, (H, W, 4)).copy(), np.broadcast_to(Hc, (H, W, 4)).copy()
    for blend in (1, 26, 255):
        nn = (Hc[:3].astype(np.int64) * (256 - blend) + Cc[:3].astype(np.int64) * 256 * blend + 128) >> 8
        out, hout = fn(ta.Case("flat_noclamp", ivp, cur, cur, depth, flat, flat_h, blend=blend, flags=ta.NO_CLAMP))
        assert (hout[..., :3] == nn).all() and (hout[..., 3] == 256 * 33).all()
        assert (out[..., :3] == np.minimum((nn + 128) >> 8, 255)).all() and (out[..., 3] == 33).all()
        out, hout = fn(ta.Case("flat_clamp", ivp, cur, cur, depth, flat, flat_h, blend=blend))
        assert np.array_equal(out, flat) and (hout == flat.astype(np.uint16) * 256).all()
    # W = 64, NDC x translated by 2 k / 64: the history comes from exactly k texels to the side with fx == fy == 0
    W, H = 64, 9
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    hist = ta.make_history("random", img, rng)
    depth = ta.make_depth("random", W, H, rng)
    for k in (1, -3, 40):
        ivp, cur, prev = ta.translate_matrices(k, W)
        out, hout = fn(ta.Case("translate", ivp, cur, prev, depth, img, hist, blend=128, flags=ta.NO_CLAMP))
        src = np.arange(W) + k
        has = (src >= 0) & (src <= W - 1)
        want = img.astype(np.int64) * 256
        blended = (hist[:, np.clip(src, 0, W - 1), :3].astype(np.int64) * 128 + img[..., :3].astype(np.int64) * 256 * 128 + 128) >> 8
        want[:, has, :3] = blended[:, has]
        assert np.array_equal(hout, want.astype(np.uint16)), k
        assert np.array_equal(out[..., :3], np.minimum((want[..., :3] + 128) >> 8, 255)) and np.array_equal(out[..., 3], img[..., 3])


def test_known_answers(built_lib):
    answers(lambda c: ta.checker(c)[:2])
    answers(lambda c: run_host(c))
    answers(lambda c: run_host(c, misalign=12))


def tall_case(motion):
    rng = np.random.default_rng(190)
    W, H = 45, 190
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    ivp, cur, prev = ta.motion_matrices(motion, W, H)
    return ta.Case("tall_" + motion, ivp, cur, prev, ta.make_depth("random", W, H, rng), img, ta.make_history("random", img, rng))


SPLITS = [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 189, 190)]


@pytest.mark.parametrize("split", SPLITS)
def test_row_ranges_stitch_to_the_whole_frame(built_lib, split):
    for motion in ("dolly", "subpixel_pan"):
        case = tall_case(motion)
        whole_out, whole_hist, _ = ta.checker(case)
        s_out, s_hist = np.full_like(whole_out, ta.GUARD), np.full_like(whole_hist, ta.GUARD * 257)
        for row0, end in zip(split[:-1], split[1:]):
            out, hist = run_host(case, row0=row0, rows=end - row0)
            ref_out, ref_hist, _ = ta.checker(case, row0=row0, rows=end - row0)
            assert np.array_equal(out, ref_out) and np.array_equal(hist, ref_hist), (motion, row0, end)
            for plane, guard in ((out, ta.GUARD), (hist, ta.GUARD * 257)):
                assert (plane[:row0] == guard).all() and (plane[end:] == guard).all(), "rows outside the range were written"
            s_out[row0:end], s_hist[row0:end] = out[row0:end], hist[row0:end]
        assert np.array_equal(s_out, whole_out) and np.array_equal(s_hist, whole_hist), motion
    out, hist = run_host(case, row0=190, rows=0)
    assert (out == ta.GUARD).all() and (hist == ta.GUARD * 257).all()


def test_default_params(built_lib):
    p = built_lib.TaaParams()
    assert C.sizeof(p) == 32 and built_lib.lib.crychic_taa_default_params(C.byref(p)) == 0
    assert (p.blend, p.flags, tuple(p.reserved)) == (26, 0, (0,) * 6)
    assert built_lib.lib.crychic_taa_default_params(None) == -1
    assert (built_lib.TAA_RESET, built_lib.TAA_NO_CLAMP) == (1, 2)
    q = built_lib.TaaParams.default(blend=64, flags=built_lib.TAA_NO_CLAMP)
    assert (q.blend, q.flags) == (64, 2)
    assert built_lib.lib.crychic_taa_history_bytes(70, 38) == 70 * 38 * 8 and built_lib.lib.crychic_taa_history_bytes(1 << 16, 1 << 12) == 1 << 31


# ---- the jitter and the jittered builders ---------------------------------------------------------------------------------------------

def radical_inverse(i, base):
    r, f = Fraction(0), Fraction(1, base)
    while i:
        r += (i % base) * f
        i //= base
        f /= base
    return r


def test_jitter_against_exact_rationals(built_lib):
    """jx = r2 - 1/2 exactly; jy = fl(fl(n / d) - 0.5) with n / d the base-3 radical inverse over the denominator of its digits: numpy's
    float32 division and subtraction are the IEEE operations the header names."""
    seen = []
    for index in list(range(40)) + [0xFFFFFFFF, 0xFFFFFFF0]:
        jx, jy = ta.jitter(index)
        i = 1 + index % 16
        assert Fraction(jx) == radical_inverse(i, 2) - Fraction(1, 2)
        r3 = radical_inverse(i, 3)
        d = 3 if i < 3 else (9 if i < 9 else 27)
        n = r3 * d
        assert n.denominator == 1
        want = np.float32(np.float32(int(n)) / np.float32(d)) - np.float32(0.5)
        assert np.float32(jy) == want and abs(Fraction(jy) - (r3 - Fraction(1, 2))) <= Fraction(1, 1 << 24)
        assert -0.5 <= jx < 0.5 and -0.5 <= jy < 0.5
        seen.append((jx, jy))
    assert seen[:16] == seen[16:32] and len(set(seen[:16])) == 16
    assert built_lib.lib.crychic_taa_jitter(0, None, None) == -1


def both_constants(lib, W, H, jx, jy, cam=None):
    from crychic_renderer_amd import scene
    consts = scene.Constants(W, H, 64, cam=cam, jitter=(jx, jy))
    return consts.pass_cb, consts.ssao_cb


def test_zero_jitter_is_the_unjittered_builders_byte_for_byte(built_lib):
    from crychic_renderer_amd import scene
    lib = built_lib.lib
    for W, H, cam in ((1920, 1080, None), (70, 38, None), (3840, 2160, scene.covered_camera(3840, 2160))):
        c = scene.Constants(W, H, 64, cam=cam)
        dirs = np.asarray(scene.BASE_LIGHT_DIRS, np.float32)
        for jx, jy in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0)):
            plain, jit = built_lib.PassConstants(), built_lib.PassConstants()
            assert lib.crychic_update_main_pass_cb(C.byref(c.cam), W, H, c.shadow_transform.ctypes.data, dirs.ctypes.data, C.byref(plain)) == 0
            assert lib.crychic_update_main_pass_cb_jittered(C.byref(c.cam), W, H, c.shadow_transform.ctypes.data, dirs.ctypes.data, jx, jy, C.byref(jit)) == 0
            assert bytes(plain) == bytes(jit) == bytes(c.pass_cb)
            splain, sjit = built_lib.SsaoConstants(), built_lib.SsaoConstants()
            assert lib.crychic_update_ssao_cb(C.byref(c.cam), W, H, C.cast(c.offsets, C.c_void_p), C.byref(splain)) == 0
            assert lib.crychic_update_ssao_cb_jittered(C.byref(c.cam), W, H, C.cast(c.offsets, C.c_void_p), jx, jy, C.byref(sjit)) == 0
            assert bytes(splain) == bytes(sjit) == bytes(c.ssao_cb)
    bad = built_lib.PassConstants()
    assert lib.crychic_update_main_pass_cb_jittered(C.byref(c.cam), 70, 38, c.shadow_transform.ctypes.data, dirs.ctypes.data, math.nan, 0.0, C.byref(bad)) == -1
    assert lib.crychic_update_ssao_cb_jittered(C.byref(c.cam), 70, 38, C.cast(c.offsets, C.c_void_p), 0.0, math.inf, C.byref(splain)) == -1


def project(m16, p):
    """Pixel position of world point p (float64) through a stored-transposed view-projection on a W x H frame, up to the frame's size."""
    m = np.asarray(m16, np.float64).reshape(4, 4)        # row c = column c of the row-vector matrix
    h = m @ np.append(np.asarray(p, np.float64), 1.0)
    return h[0] / h[3], h[1] / h[3], h[3]


def test_jittered_view_proj_moves_a_point_by_the_jitter(built_lib):
    """A world point lands (jx, jy) pixels from its unjittered position.  Tolerance: the matrices' entries are binary32, each the
    rounded sum of four rounded products (about 4 half-ulps, 2^-22 relative); a pixel position is W / 2 times an NDC coordinate of
    magnitude at most 1 whose numerator and denominator each carry that error over three terms, so 2^-19 W pixels covers it (0.0037
    pixels at 1920) with room to spare; the evaluation itself is in float64."""
    rng = np.random.default_rng(3)
    for W, H in ((1920, 1080), (70, 38)):
        tol = W * 2.0 ** -19
        for index in range(16):
            jx, jy = ta.jitter(index)
            plain, _ = both_constants(built_lib, W, H, 0.0, 0.0)
            jit, sjit = both_constants(built_lib, W, H, jx, jy)
            for _ in range(8):
                p = rng.uniform((-20, 0, -5), (20, 6, 60))
                x0, y0, w0 = project(plain.ViewProj, p)
                x1, y1, w1 = project(jit.ViewProj, p)
                assert w0 > 1.0 and w1 == w0
                px0, py0 = (x0 + 1) * 0.5 * W, (1 - y0) * 0.5 * H
                px1, py1 = (x1 + 1) * 0.5 * W, (1 - y1) * 0.5 * H
                assert abs((px1 - px0) - jx) <= tol and abs((py1 - py0) - jy) <= tol, (W, index, px1 - px0, py1 - py0, jx, jy)
            # every field that depends on Proj was rebuilt from the shifted matrix
            P, V = np.asarray(jit.Proj, np.float64).reshape(4, 4).T, np.asarray(jit.View, np.float64).reshape(4, 4).T
            assert np.allclose(V @ P, np.asarray(jit.ViewProj, np.float64).reshape(4, 4).T, rtol=1e-5, atol=1e-5)
            assert np.allclose(np.asarray(jit.InvProj, np.float64).reshape(4, 4).T @ P, np.eye(4), atol=1e-4)
            assert np.allclose(np.asarray(jit.InvViewProj, np.float64).reshape(4, 4).T @ (V @ P), np.eye(4), atol=1e-3)
            assert bytes(sjit.Proj) == bytes(jit.Proj) and bytes(sjit.InvProj) == bytes(jit.InvProj)
            T = np.array([[0.5, 0, 0, 0], [0, -0.5, 0, 0], [0, 0, 1, 0], [0.5, 0.5, 0, 1]])
            assert np.allclose(V @ P @ T, np.asarray(jit.ViewProjTex, np.float64).reshape(4, 4).T, rtol=1e-5, atol=1e-5)
            assert np.allclose(P @ T, np.asarray(sjit.ProjTex, np.float64).reshape(4, 4).T, rtol=1e-5, atol=1e-5)
            assert (jx == 0.0 or plain.Proj[2] != jit.Proj[2]) and (jy == 0.0 or plain.Proj[6] != jit.Proj[6])


def test_jittered_raycaster_agrees_with_the_jittered_view_proj(built_lib):
    """The near top corners of the box at (0, 0.8, -5), facing the reference camera: projected through the jittered ViewProj a corner
    falls between pixel centres, and the pixel diagonally inside the box from that position is shaded with the box (its g0 holds a
    point of the box's front face) while the one diagonally outside is not."""
    from crychic_renderer_amd import scene
    W, H = 320, 180
    for index in (0, 1, 2, 5, 7, 12):
        jx, jy = ta.jitter(index)
        consts = scene.Constants(W, H, 64, jitter=(jx, jy))
        g0 = scene._camera_planes(consts, "cpu")["g0"].numpy()
        on_face = (np.abs(g0[..., 2] - (-5.8)) < 1e-3) & (np.abs(g0[..., 0]) <= 0.8 + 1e-3) & (g0[..., 1] <= 1.6 + 1e-3) & (g0[..., 3] == 0.5)
        for sign in (-1.0, 1.0):
            x, y, _ = project(consts.pass_cb.ViewProj, (sign * 0.8, 1.6, -5.8))
            sx, sy = (x + 1) * 0.5 * W, (1 - y) * 0.5 * H                  # pixel (px, py) covers [px, px + 1) x [py, py + 1), centre + 0.5
            # nearest pixel centres strictly inside / outside the corner, at least a hundredth of a pixel away from the edge
            lo_x, hi_x = math.floor(sx - 0.5 - 0.01), math.ceil(sx - 0.5 + 0.01)
            ix, ox = (lo_x, hi_x) if sign > 0 else (hi_x, lo_x)
            iy, oy = math.ceil(sy - 0.5 + 0.01), math.floor(sy - 0.5 - 0.01)
            assert on_face[iy, ix], (index, sign, sx, sy)
            assert not on_face[iy, ox] and not on_face[oy, ix], (index, sign, sx, sy)


def test_convergence_on_the_still_scene(built_lib):
    """16 jittered frames of the still reference scene lit by the oracle at 160 x 90 and resolved by the checker, against a 640 x 360
    frame box-filtered 4 x 4: over the edge pixels -- those where the single unjittered frame differs from the truth -- the resolved
    frame's mean absolute RGBA8 error is lower than the unjittered frame's."""
    W, H = 160, 90
    small = ta.StillScene(W, H)
    plain = small.frame()[0].astype(np.int32)
    resolved = small.resolve(16).astype(np.int32)
    truth = ta.box_filter(ta.StillScene(4 * W, 4 * H).frame()[0], 4)
    edge = (plain != truth).any(-1)
    e_plain, e_taa = np.abs(plain - truth)[edge].mean(), np.abs(resolved - truth)[edge].mean()
    print("edge pixels %.1f %%: mean absolute error %.4f unjittered, %.4f resolved" % (100.0 * edge.mean(), e_plain, e_taa))
    assert edge.any() and e_taa < e_plain


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, P = built_lib.lib, built_lib.TaaParams
    W, H = 64, 32
    a, b, d, hi, ho = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000           # never dereferenced
    fb, hb = W * H * 4, W * H * 8
    good = built_lib.PassConstants()
    good.InvViewProj[:] = list(ta.IDENTITY)
    eye = (C.c_float * 16)(*ta.IDENTITY)

    def mat(k, v):
        m = (C.c_float * 16)(*ta.IDENTITY)
        m[k] = v
        return m

    def call(cb=good, cur=eye, prev=eye, depth=d, src=a, hin=hi, hout=ho, dst=b, W=W, H=H, row0=0, rows=H, params=None):
        rc = lib.crychic_taa(None, None if cb is None else C.byref(cb), cur, prev, depth, src, hin, hout, dst, W, H, row0, rows,
                             None if params is None else C.byref(params), None)
        return rc, lib.crychic_last_error().decode()

    ok = (-1, "null context")
    assert call() == ok
    assert call(dst=a + fb) == ok and call(hout=hi + hb) == ok and call(hin=a + fb, dst=a + fb + hb) == ok, "adjacent planes do not overlap"
    assert call(row0=H, rows=0) == ok and call(W=1, H=1, rows=1) == ok
    assert call(params=P.default(blend=1)) == ok and call(params=P.default(blend=256, flags=3)) == ok
    assert call(hin=None, params=P.default(flags=ta.RESET)) == ok, "history_in may be NULL with RESET"
    assert call(hin=hi + 8, hout=ho + 8, src=a + 4, dst=b + 4, depth=d + 12) == ok
    bad_res = P.default()
    bad_res.reserved[5] = 1
    bad_cb = built_lib.PassConstants.from_buffer_copy(good)
    bad_cb.InvViewProj[7] = math.inf
    for kw, word in ((dict(cb=None), "null argument"), (dict(cur=None), "null argument"), (dict(prev=None), "null argument"),
                     (dict(depth=None), "null argument"), (dict(src=None), "null argument"), (dict(hin=None), "null argument"),
                     (dict(hout=None), "null argument"), (dict(dst=None), "null argument"),
                     (dict(hout=None, params=P.default(flags=ta.RESET)), "null argument"),
                     (dict(src=a + 2), "4-byte aligned"), (dict(dst=b + 1), "4-byte aligned"), (dict(depth=d + 2), "4-byte aligned"),
                     (dict(hin=hi + 4), "8-byte aligned"), (dict(hout=ho + 4), "8-byte aligned"),
                     (dict(W=0), "non-zero"), (dict(H=0, rows=0), "non-zero"),
                     (dict(row0=H + 1, rows=0), "outside the 32-row frame"), (dict(row0=1, rows=H), "outside the 32-row frame"),
                     (dict(row0=0xFFFFFFFF, rows=2), "outside the 32-row frame"),
                     (dict(cb=bad_cb), "not finite"), (dict(cur=mat(0, math.nan)), "not finite"), (dict(prev=mat(15, -math.inf)), "not finite"),
                     (dict(params=P.default(blend=0)), "blend"), (dict(params=P.default(blend=257)), "blend"),
                     (dict(params=P.default(flags=4)), "flags"), (dict(params=P.default(flags=0x80000001)), "flags"), (dict(params=bad_res), "reserved"),
                     (dict(dst=a), "overlap"), (dict(dst=a + 4), "overlap"), (dict(dst=a + fb - 4), "overlap"), (dict(src=b + fb - 4), "overlap"),
                     (dict(hout=hi), "history planes overlap"), (dict(hout=hi + hb - 8), "history planes overlap"),
                     (dict(hin=ho + hb - 8), "history planes overlap"),
                     (dict(hout=hi, params=P.default(flags=ta.RESET)), "history planes overlap"),
                     (dict(hin=a + fb - 8), "overlaps a frame plane"), (dict(hout=b + 8), "overlaps a frame plane"), (dict(hout=d + fb - 8), "overlaps a frame plane"),
                     (dict(hin=b - hb + 8), "overlaps a frame plane"), (dict(hout=a, params=P.default(flags=ta.RESET), hin=None), "overlaps a frame plane")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = call(W=1 << 15, H=(1 << 13) + 1, rows=1)
    assert rc == -4 and "exceeds" in msg
    rc, msg = call(W=(1 << 22) + 1, H=1, rows=1)
    assert rc == -4 and "2^22" in msg
    assert call(W=1 << 22, H=1, rows=1) == ok
