"""crychic_dof on the CPU tier: the kernel body (csrc/dof_core.hpp, built for the host with the workgroup, the LDS window, the barrier
and the lane walk emulated) against the checker (tests/dof_ref, plain C from the definition in include/crychic_hip.h), byte for byte
on the whole corpus, behind guard bytes and on misaligned planes; what the corpus must reach, checked with the checker alone; the
definition's tables and its sum bound; its five known answers; row ranges; and the refusals of the real library, which need no
device."""
import ctypes as C
import math

import numpy as np
import pytest

import dof_host_lib as host
import dof_lib as dl


@pytest.fixture(scope="module")
def cases(built_lib):
    return dl.corpus()


def run_host(frame, img, params=None, row0=0, rows=None, misalign=0):
    """The kernel body on guarded copies of `img` and of the depth plane, `misalign` bytes past a 16-byte boundary: the output plane;
    asserts the guard bytes around the planes and that nothing but `out` changed."""
    sraw, src = dl.guarded(img.shape, misalign=misalign)
    draw, depth = dl.guarded(frame.depth.shape, np.uint32, misalign=misalign)
    oraw, out = dl.guarded(img.shape, misalign=misalign)
    src[...] = img
    depth[...] = frame.depth
    f = dl.Frame((frame.A, frame.B), depth)
    assert f.depth.ctypes.data == depth.ctypes.data and depth.ctypes.data % 16 == misalign
    host.dof(f, src, out, params, row0, rows)
    assert dl.guards_intact(sraw, src) and dl.guards_intact(oraw, out) and dl.guards_intact(draw, depth), "guard bytes changed"
    assert np.array_equal(depth, frame.depth) and np.array_equal(src, img), "an input plane changed"
    return out


@pytest.mark.parametrize("pname", list(dl.PARAM_SETS))
def test_host_body_equals_checker(cases, pname):
    ran = 0
    for name, frame, img, pn, _ in cases:
        if pn != pname:
            continue
        ref, _ = dl.expected(name)
        for misalign in (0, 4, 12):
            got = run_host(frame, img, dl.PARAM_SETS[pn], misalign=misalign)
            assert np.array_equal(got, ref), "%s, planes %d bytes past a 16-byte boundary: %d bytes differ" % (name, misalign, int((got != ref).sum()))
        ran += 1
    assert ran >= 1


def test_the_corpus_reaches_what_it_must(cases):
    """With the checker alone: every size, R, aperture, depth kind and both projections are there, the focus distance lies in front
    of, inside and behind the scene, and every branch the checker counts is taken."""
    assert {img.shape[1::-1] for _, _, img, _, _ in cases} >= set(dl.SIZES) | {(64, 64), (128, 96)}
    used = [dl.PARAM_SETS[p] for _, _, _, p, _ in cases]
    assert {p["radius"] for p in used} >= {1, 2, 5, 8} and {p["aperture"] for p in used} >= {0.0, 0.5, 6.0, 64.0}
    assert min(p["focus"] for p in used) < 5.0 and max(p["focus"] for p in used) > 40.0 and any(5.0 < p["focus"] < 40.0 for p in used)
    assert {p for _, _, _, p, _ in cases} == set(dl.PARAM_SETS)
    assert {k for _, _, _, _, k in cases} == set(dl.DEPTH_KINDS) | {"rendered"}
    assert {(f.A, f.B) for _, f, _, _, _ in cases} >= {tuple(map(dl.f32, dl.REFERENCE_AB)), tuple(map(dl.f32, dl.OTHER_AB))}
    for W, H in dl.SIZES:
        assert {k for _, _, img, _, k in cases if img.shape[1::-1] == (W, H)} >= set(dl.DEPTH_KINDS)
    total = dict.fromkeys(dl.COUNTERS, 0)
    discs = dl.tables()[0]
    for name, frame, img, pname, _ in cases:
        _, n = dl.expected(name)
        H, W = img.shape[:2]
        taps = W * H * discs[dl.PARAM_SETS[pname]["radius"] - 1]
        assert n["c_zero"] + n["c_interior"] + n["c_hi"] == W * H, name
        assert n["tap_outside"] + n["behind"] + n["not_behind"] == taps, name
        assert n["k_zero"] + n["k_interior"] + n["k_sixteen"] == n["ce_below_16"] + n["ce_in_inv"] == n["behind"] + n["not_behind"], name
        for k in total:
            total[k] += n[k]
    assert all(v > 0 for v in total.values()), total
    assert dl.expected("nan_clamp")[1]["clamp_nan"] == 65 * 7
    for name in ("golden64_default", "scene128_default"):       # the rendered frames hold sharp and blurred texels, near and far taps
        n = dl.expected(name)[1]
        assert min(n["behind"], n["not_behind"], n["k_zero"], n["k_interior"], n["k_sixteen"], n["c_interior"]) > 0, (name, n)


def test_tables_and_the_sum_bound(built_lib):
    """The definition's tables from the checker, the kernel's tap table against them, and the bound that keeps the sums in 32 bits."""
    discs, inv, d16 = dl.tables()
    assert discs == [5, 13, 29, 49, 81, 113, 149, 197]
    assert inv[:17] == [4096] * 17 and (inv[17], inv[64], inv[128]) == (3628, 256, 64) and len(inv) == 129
    assert all(a >= b for a, b in zip(inv, inv[1:])), "inv[] rises somewhere: min(c_s, c_p) would not be the larger inv"
    assert all(v == math.isqrt(256 * (ox * ox + oy * oy)) for (ox, oy), v in d16.items()) and max(d16.values()) == 128
    # the largest weight, channel sum and rounding term, and the smallest sum of weights (the centre tap alone)
    wmax = max(min(max(c + 8 - d, 0), 16) * inv[c] for c in range(129) for d in set(d16.values()))
    assert wmax == 16 * 4096
    assert 197 * wmax * 255 == 3292200960 and 3292200960 + ((197 * wmax) >> 1) < 1 << 32
    assert min(min(c + 8, 16) * inv[c] for c in range(129)) == 1024
    # the kernel's table: the same offsets, sorted so that every disc is a prefix and d16 never falls; the sentinel ends any cut
    taps, sentinel, count = host.taps()
    assert sorted((ox, oy) for _, ox, oy in taps) == sorted(d16) and all(d == d16[(ox, oy)] for d, ox, oy in taps)
    assert taps[0] == (0, 0, 0) and all(a[0] <= b[0] for a, b in zip(taps, taps[1:])) and sentinel >> 16 > 128 + 8
    assert count[1:] == discs
    for R in range(1, 9):
        assert all(ox * ox + oy * oy <= R * R for _, ox, oy in taps[:count[R]]) and all(ox * ox + oy * oy > R * R for _, ox, oy in taps[count[R]:])


def step_frames():
    """The two depth steps of the known answers on a 96 x 40 frame, with the parameters that put c = 0 on one side and c = 128 on the
    other: (frame, params, columns of the near half, columns of the far half)."""
    rng = np.random.default_rng(3)
    W, H = 96, 40
    sharp_near = (dl.Frame(dl.REFERENCE_AB, dl.make_depth("step_near_left", W, H, rng)), dict(focus=10.0, aperture=64.0, radius=8))
    blurred_near = (dl.Frame(dl.REFERENCE_AB, dl.make_depth("step_near_left", W, H, rng)), dict(focus=100.0, aperture=64.0, radius=8))
    near, far = int(sharp_near[0].depth[0, 0]), int(sharp_near[0].depth[0, W - 1])
    assert (dl.coc_of(*sharp_near, near), dl.coc_of(*sharp_near, far)) == (0, 128)
    assert (dl.coc_of(*blurred_near, near), dl.coc_of(*blurred_near, far)) == (128, 0)
    return sharp_near, blurred_near, W // 2


def answers(fn):
    """The definition's five known answers for fn(frame, img, params) -> the blurred frame."""
    rng = np.random.default_rng(7)
    sc = dl.scene_frame()
    img = rng.integers(0, 256, (96, 128, 4), dtype=np.uint8)
    # (a) aperture 0: out == in
    for R in (1, 5, 8):
        assert np.array_equal(fn(sc, img, dict(focus=15.0, aperture=0.0, radius=R)), img)
    # (b) one colour stays that colour, whatever the depth and the parameters; alpha is the pixel's own
    flat = np.empty((96, 128, 4), np.uint8)
    flat[..., :3] = (201, 7, 255)
    flat[..., 3] = img[..., 3]
    noise = dl.Frame(dl.OTHER_AB, dl.make_depth("random", 128, 96, rng))
    for frame, p in ((sc, dl.DEFAULTS), (noise, dict(focus=3.0, aperture=64.0, radius=8)), (noise, dict(focus=200.0, aperture=1.5, radius=3))):
        assert np.array_equal(fn(frame, flat, p), flat)
    # (c) a sharp foreground in front of a blurred background is not polluted; (d) a blurred foreground bleeds 8 columns, no further
    sharp_near, blurred_near, mid = step_frames()
    pic = rng.integers(0, 256, (40, 96, 4), dtype=np.uint8)
    out = fn(sharp_near[0], pic, sharp_near[1])
    assert np.array_equal(out[:, :mid], pic[:, :mid]) and not np.array_equal(out[:, mid:], pic[:, mid:])
    assert np.array_equal(out[..., 3], pic[..., 3])
    out = fn(blurred_near[0], pic, blurred_near[1])
    assert np.array_equal(out[:, mid + 8:], pic[:, mid + 8:]) and not np.array_equal(out[:, :mid], pic[:, :mid])
    assert all((out[:, mid + k, :3] != pic[:, mid + k, :3]).any() for k in range(8)), "a column within 8 of the step came back unchanged"
    # (e) constant depth, an input with the eight symmetries of the square lattice: so is the output
    q = rng.integers(0, 256, (20, 20, 4), dtype=np.uint8)
    q = np.maximum(q, q.transpose(1, 0, 2))                                         # symmetric under the diagonal
    half = np.concatenate([q, q[:, ::-1]], axis=1)
    sym = np.ascontiguousarray(np.concatenate([half, half[::-1]], axis=0))          # and under both mirrors: the whole group
    level = dl.Frame(dl.REFERENCE_AB, np.full((40, 40), dl.depth_word(dl.REFERENCE_AB, 30.0), np.uint32))
    out = fn(level, sym, dict(focus=10.0, aperture=9.0, radius=8))
    assert not np.array_equal(out, sym)
    for other in (out[::-1], out[:, ::-1], out.transpose(1, 0, 2), out[::-1, ::-1].transpose(1, 0, 2)):
        assert np.array_equal(out, other)


def test_known_answers(built_lib):
    answers(lambda f, i, p: dl.checker(f, i, p)[0])
    answers(lambda f, i, p: run_host(f, i, p))
    answers(lambda f, i, p: run_host(f, i, p, misalign=4))


# odd starts and odd lengths, ranges shorter than R = 8 and of one row, cuts inside and between the 16-row tiles
SPLITS = [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 96, 101, 190), (0, 16, 31, 189, 190)]


@pytest.mark.parametrize("split", SPLITS)
def test_row_ranges_stitch_to_the_whole_frame(cases, split):
    by_name = {c[0]: c for c in cases}
    for name in (dl.case_name("322x190_random"), "322x190_step_near_blurred"):
        _, frame, img, pname, _ = by_name[name]
        whole, _ = dl.expected(name)
        stitched = np.full(img.shape, dl.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got = run_host(frame, img, dl.PARAM_SETS[pname], row0=row0, rows=end - row0)
            assert (got[:row0] == dl.GUARD).all() and (got[end:] == dl.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
        assert np.array_equal(stitched, whole), name
    assert (run_host(by_name["scene128_default"][1], by_name["scene128_default"][2], dl.DEFAULTS, row0=96, rows=0) == dl.GUARD).all()


def test_a_call_reads_only_its_rows_and_the_apron(cases):
    """Rows [row0 - R, row0 + rows + R) and nothing else: the planes are inverted everywhere else."""
    _, frame, img, pname, _ = {c[0]: c for c in cases}["scene128_default"]
    whole, _ = dl.expected("scene128_default")
    for R in (8, 2):
        p = dict(dl.DEFAULTS, radius=R)
        want = whole if R == 8 else dl.checker(frame, img, p)[0]
        other, depth = np.array(img), frame.depth.copy()
        for plane in (other, depth):
            plane[:21 - R] ^= 0xFF
            plane[30 + R:] ^= 0xFF
        got = run_host(dl.Frame((frame.A, frame.B), depth), other, p, row0=21, rows=9)
        assert np.array_equal(got[21:30], want[21:30])


def test_default_params(built_lib):
    p = built_lib.DofParams()
    assert C.sizeof(p) == 32 and built_lib.lib.crychic_dof_default_params(C.byref(p)) == 0
    assert (p.focusDistance, p.aperture, p.maxRadius) == (15.0, 6.0, 8) and tuple(p.reserved) == (0, 0, 0, 0, 0)
    assert built_lib.lib.crychic_dof_default_params(None) == -1
    assert built_lib.DOF_MAX_RADIUS == 8
    q = built_lib.DofParams.default(focus=22.5, aperture=3, radius=4)
    assert (q.focusDistance, q.aperture, q.maxRadius) == (22.5, 3.0, 4)


def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, P = built_lib.lib, built_lib.DofParams
    a, b, d = 0x10000000, 0x20000000, 0x30000000           # never dereferenced
    good = dl.Frame(dl.REFERENCE_AB, np.zeros((1, 1), np.uint32)).pass_constants(built_lib)

    def call(cb=good, depth=d, src=a, dst=b, W=64, H=32, row0=0, rows=32, params=None):
        rc = lib.crychic_dof(None, None if cb is None else C.byref(cb), depth, src, dst, W, H, row0, rows,
                             None if params is None else C.byref(params), None)
        return rc, lib.crychic_last_error().decode()

    def prm(**kw):
        return P.default(**kw)

    def proj(A, B):
        cb = built_lib.PassConstants.from_buffer_copy(good)
        cb.Proj[10], cb.Proj[11] = A, B
        return cb
    assert call() == (-1, "null context")
    assert call(dst=a + 64 * 32 * 4) == (-1, "null context"), "adjacent planes do not overlap"
    assert call(row0=32, rows=0) == (-1, "null context") and call(W=1, H=1, rows=1) == (-1, "null context")
    assert call(params=prm(aperture=0.0, radius=1)) == (-1, "null context") and call(params=prm(aperture=64.0, focus=3e38)) == (-1, "null context")
    assert call(cb=proj(-3.0e38, 1.0e-30)) == (-1, "null context")
    bad_res = prm()
    bad_res.reserved[4] = 1
    for kw, word in ((dict(cb=None), "null argument"), (dict(depth=None), "null argument"), (dict(src=None), "null argument"), (dict(dst=None), "null argument"),
                     (dict(src=a + 2), "aligned"), (dict(dst=b + 1), "aligned"), (dict(depth=d + 2), "aligned"),
                     (dict(W=0), "non-zero"), (dict(H=0, rows=0), "non-zero"),
                     (dict(row0=33, rows=0), "outside the 32-row frame"), (dict(row0=1, rows=32), "outside the 32-row frame"),
                     (dict(row0=0xFFFFFFFF, rows=2), "outside the 32-row frame"),
                     (dict(params=prm(focus=0.0)), "focusDistance"), (dict(params=prm(focus=-1.0)), "focusDistance"),
                     (dict(params=prm(focus=math.inf)), "focusDistance"), (dict(params=prm(focus=math.nan)), "focusDistance"),
                     (dict(params=prm(aperture=-0.5)), "aperture"), (dict(params=prm(aperture=64.5)), "aperture"),
                     (dict(params=prm(aperture=math.nan)), "aperture"), (dict(params=prm(aperture=math.inf)), "aperture"),
                     (dict(params=prm(radius=0)), "maxRadius"), (dict(params=prm(radius=9)), "maxRadius"), (dict(params=bad_res), "reserved"),
                     (dict(cb=proj(math.nan, -1.0)), "Proj[10]"), (dict(cb=proj(math.inf, -1.0)), "Proj[10]"), (dict(cb=proj(1.0, math.nan)), "Proj[11]"),
                     (dict(cb=proj(1.0, -math.inf)), "Proj[11]"), (dict(cb=proj(1.0, 0.0)), "Proj[11]"), (dict(cb=proj(1.0, -0.0)), "Proj[11]"),
                     (dict(dst=a), "overlap"), (dict(dst=a + 4), "overlap"), (dict(dst=a + 64 * 32 * 4 - 4), "overlap"),
                     (dict(src=b + 64 * 32 * 4 - 4), "overlap")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = call(W=1 << 15, H=(1 << 13) + 1, rows=1)
    assert rc == -4 and "exceeds" in msg
    assert call(W=1 << 15, H=1 << 13, rows=1, dst=a + (1 << 30)) == (-1, "null context")        # 2^28 pixels
