"""crychic_grade on the CPU: the known answers that tell misreadings of the definition (include/crychic_hip.h) apart; the host build
of the kernel's body (tests/grade_host) against the checker (tests/grade_ref) and the numpy restatement (tests/grade_restate.py),
every byte of every case; the table builder against a float64 restatement; the .cube loader; and the refusals, which need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import grade_host_lib as gh
import grade_lib as gl
import grade_restate as gr


# ---- known answers: `run(img, lut) -> frame` is the checker here and the device in tests/test_grade_gpu.py ----------------------------

def answers(run):
    frame = gl.all_values_frame()
    # the identity table is exact where N - 1 divides 255
    for N in (2, 16, 18):
        assert np.array_equal(run(frame, gl.identity_lut(N)), frame), "the identity table of size %d changes the frame" % N
    # elsewhere an entry is off by at most 1/2, the combination is convex and the last rounding adds at most 1/2
    for N in (17, 33):
        d = np.abs(run(frame, gl.identity_lut(N)).astype(int) - frame)
        assert d.max() <= 1, "the identity table of size %d moves a byte by %d" % (N, d.max())
    for N in (2, 16):
        got = run(frame, gl.lut_from(lambda r, g, b: (255 - r, 255 - g, 255 - b), N))
        assert np.array_equal(got[..., :3], 255 - frame[..., :3]) and np.array_equal(got[..., 3], frame[..., 3]), "inverting table, N = %d" % N
        got = run(frame, gl.lut_from(lambda r, g, b: (b, r, g), N))
        assert np.array_equal(got[..., :3], frame[..., [2, 0, 1]]), "channel-swapping table, N = %d" % N
    # white at (1, 1, 1) alone: tetrahedral interpolation gives min(R, G, B), trilinear R G B / 255^2
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (9, 31, 4), dtype=np.uint8)
    corner = np.zeros((2, 2, 2, 4), np.uint8)
    corner[1, 1, 1] = 255
    got = run(noise, corner)
    assert np.array_equal(got[..., :3], np.repeat(noise[..., :3].min(axis=2, keepdims=True), 3, axis=2)), "the white-corner table does not give min(R, G, B)"
    assert np.array_equal(got[..., 3], noise[..., 3]), "alpha does not survive"
    # the byte that is never looked at
    lut = gl.corpus_lut(17)
    other = lut.copy()
    other[..., 3] = rng.integers(0, 256, other.shape[:3], dtype=np.uint8)
    assert np.array_equal(run(noise, lut), run(noise, other)), "the fourth byte of an entry reaches the output"
    # v = 255 reads cell N - 2 with f = 255: the far corner's entry, and nothing of its neighbours
    for N in (2, 17, 33):
        lut = gl.corpus_lut(N).copy()
        white = np.full((1, 5, 4), 255, np.uint8)
        assert (run(white, lut)[..., :3] == lut[N - 1, N - 1, N - 1, :3]).all()
        lut[N - 2] ^= 0xFF
        lut[:, N - 2] ^= 0xFF
        lut[:, :, N - 2] ^= 0xFF
        assert (run(white, lut)[..., :3] == lut[N - 1, N - 1, N - 1, :3]).all(), "white looks at an entry other than the far corner's"


def test_known_answers_checker():
    answers(lambda img, lut: gl.checker(img, lut))


def test_known_answers_restatement():
    answers(lambda img, lut: gr.apply(img, lut))


def _cases():
    """(name, frame, table): random frames and tables, every value of every channel, the tie frames, white and black."""
    out = []
    for N in gl.SIZES:
        out.append(("67x5 N=%d" % N, gl.frame(67, 5), gl.corpus_lut(N)))
        out.append(("all values N=%d" % N, gl.all_values_frame(), gl.corpus_lut(N)))
        out.append(("ties N=%d" % N, gl.tie_frame(N), gl.corpus_lut(N)))
    out.append(("128x96 N=33", gl.frame(128, 96), gl.corpus_lut(33)))
    return out


def test_restatement_equals_checker():
    for name, img, lut in _cases():
        assert np.array_equal(gr.apply(img, lut), gl.checker(img, lut)), name


def test_tie_frames_tie():
    """Every pair of fractions ties on the tie frame of every size, with the third fraction above, below and equal."""
    for N in gl.SIZES:
        v = gl.tie_frame(N)[0, :, :3].astype(np.int64) * (N - 1)
        f = v - 255 * np.minimum(v // 255, N - 2)
        for a, b, c in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            tie = f[:, a] == f[:, b]
            assert (tie & (f[:, c] > f[:, a])).any() and (tie & (f[:, c] < f[:, a])).any() and (tie & (f[:, c] == f[:, a])).any(), (N, a, b)


@pytest.mark.parametrize("mutation", gr.MUTATIONS)
def test_restatement_bites(mutation):
    """One misreading of the header made on purpose in the restatement: a comparison with the checker must fail on the cases above.
    no_clamp gives every out-of-range vertex the weight 0, so it shows only as a lookup outside the table: that counts."""
    fails = []
    for name, img, lut in _cases():
        try:
            if not np.array_equal(gr.apply(img, lut, mutation), gl.checker(img, lut)):
                fails.append(name)
        except IndexError:
            fails.append(name + " (outside the table)")
    print("%s: %d of %d comparisons fail, the first: %s" % (mutation, len(fails), len(_cases()), fails[:1]))
    assert fails, "the cases cannot tell %s from the header's text" % mutation


def test_tie_order_is_free():
    """Breaking ties the other way round changes no byte: the header leaves the order to the implementation."""
    for name, img, lut in _cases():
        assert np.array_equal(gr.apply(img, lut, gr.SURVIVOR), gl.checker(img, lut)), name


# ---- the CPU tier: the host build of the kernel's body -------------------------------------------------------------------------------

def run_host(img, lut, misalign=0, in_place=False, ranges=None, cus=3):
    """The body over guarded planes `misalign` bytes past a 64-byte boundary: the frame, guards and input checked."""
    raw_in, src = gl.guarded(img.shape, np.uint8, misalign=misalign)
    src[...] = img
    raw_out, out = (raw_in, src) if in_place else gl.guarded(img.shape, np.uint8, misalign=misalign)
    raw_lut, table = gl.guarded(lut.shape, np.uint8, misalign=4)
    table[...] = lut
    stats = {}
    for row0, rows in ranges or [(0, img.shape[0])]:
        stats = gh.grade(src, out, table, row0, rows, cus)
    assert gl.guards_intact(raw_in, src) and gl.guards_intact(raw_out, out) and gl.guards_intact(raw_lut, table), "a guard byte changed"
    assert in_place or np.array_equal(src, img), "the input changed"
    assert np.array_equal(table, lut), "the table changed"
    return out.copy(), stats


def test_div255_is_exact():
    assert gh.div255_mismatches() == 0


def test_host_known_answers():
    answers(lambda img, lut: run_host(img, lut)[0])
    answers(lambda img, lut: run_host(img, lut, misalign=12)[0])


@pytest.mark.parametrize("N", gl.SIZES)
def test_host_equals_checker_equals_restatement(N):
    lut = gl.corpus_lut(N)
    for W, H in gl.FRAMES:
        img = gl.frame(W, H)
        ref = gl.checker(img, lut)
        if W * H <= 67 * 5:
            assert np.array_equal(gr.apply(img, lut), ref), (W, H)
        for misalign in gl.MISALIGN:
            got, stats = run_host(img, lut, misalign=misalign)
            assert np.array_equal(got, ref), "%dx%d, %d bytes past a 16-byte boundary: %d bytes differ" % (W, H, misalign, int((got != ref).sum()))
            assert stats["vec_launches"] == 1
        got, _ = run_host(img, lut, misalign=8, in_place=True)
        assert np.array_equal(got, ref), "%dx%d in place" % (W, H)
    tie = gl.tie_frame(N)
    assert np.array_equal(run_host(tie, lut)[0], gl.checker(tie, lut)), "the tie frame"


def test_host_differently_aligned_planes_take_the_narrow_path():
    img, lut = gl.frame(67, 5), gl.corpus_lut(17)
    raw_in, src = gl.guarded(img.shape, np.uint8, misalign=4)
    src[...] = img
    raw_out, out = gl.guarded(img.shape, np.uint8, misalign=8)
    stats = gh.grade(src, out, lut)
    assert stats["vec_launches"] == 0 and np.array_equal(out, gl.checker(img, lut))
    assert gl.guards_intact(raw_in, src) and gl.guards_intact(raw_out, out)


@pytest.mark.parametrize("W,H", [(67, 5), (5, 3), (3, 1)])
def test_host_row_ranges(W, H):
    """On widths that are no multiple of 4: [0, H), [1, H - 1) and a single row write their rows and no other byte."""
    img, lut = gl.frame(W, H), gl.corpus_lut(33)
    ref = gl.checker(img, lut)
    for row0, rows in gl.row_ranges(H):
        for misalign in (0, 4):
            got, _ = run_host(img, lut, misalign=misalign, ranges=[(row0, rows)])
            want = np.full_like(ref, gl.GUARD)
            want[row0:row0 + rows] = ref[row0:row0 + rows]
            assert np.array_equal(got, want), (W, H, row0, rows, misalign)
    got, _ = run_host(img, lut, ranges=[(0, 0)])
    assert (got == gl.GUARD).all(), "rows == 0 wrote"


def test_host_more_than_one_trip():
    """128 x 96 planned for one compute unit: 3 quads per lane, each workgroup a second and a third trip."""
    img, lut = gl.frame(128, 96), gl.corpus_lut(33)
    got, stats = run_host(img, lut, cus=1)
    assert stats["groups"] == 1 and np.array_equal(got, gl.checker(img, lut))
    got, stats = run_host(img, gl.corpus_lut(17), cus=1)
    assert stats["groups"] == 2 and np.array_equal(got, gl.checker(img, gl.corpus_lut(17)))


def test_refusals_need_no_device(built_lib):
    f, err = built_lib.lib.crychic_grade, built_lib.lib.crychic_last_error
    buf = np.zeros(64 * 32 * 4 * 2 + 64, np.uint8)
    lut = np.zeros(4 * 33 ** 3 + 16, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    a, b, t = C.c_void_p(base), C.c_void_p(base + 64 * 32 * 4), C.c_void_p(lut.ctypes.data + (-lut.ctypes.data) % 16)
    W, H = 64, 32
    assert f(None, a, b, W, H, 0, H, t, 1, None) == -1 and "outside 2 .. 33" in err().decode()
    assert f(None, a, b, W, H, 0, H, t, 34, None) == -1 and "outside 2 .. 33" in err().decode()
    assert f(None, None, b, W, H, 0, H, t, 17, None) == -1
    assert f(None, a, None, W, H, 0, H, t, 17, None) == -1
    assert f(None, a, b, W, H, 0, H, None, 17, None) == -1
    assert f(None, a, b, W, H, 1, H, t, 17, None) == -1 and "rows" in err().decode()
    assert f(None, a, b, W, H, H + 1, 0, t, 17, None) == -1
    assert f(None, a, b, 0, H, 0, 0, t, 17, None) == -1
    assert f(None, a, C.c_void_p(base + 16), W, H, 0, H, t, 17, None) == -1 and "overlap" in err().decode()
    assert f(None, a, C.c_void_p(base + 2), W, H, 0, H, t, 17, None) == -1 and "aligned" in err().decode()
    assert f(None, a, b, W, H, 0, H, C.c_void_p(t.value + 2), 17, None) == -1 and "table is not 4-byte aligned" in err().decode()
    assert f(None, a, b, W, H, 0, H, b, 2, None) == -1 and "table overlaps" in err().decode()
    assert f(None, a, b, 1 << 15, 1 << 14, 0, 1, t, 17, None) == -4
    # everything in order but the context: in place is not an overlap
    assert f(None, a, a, W, H, 0, H, t, 33, None) == -1 and "null context" in err().decode()
    assert f(None, a, b, W, H, 0, H, t, 2, None) == -1 and "null context" in err().decode()


# ---- the builder ---------------------------------------------------------------------------------------------------------------------

def cdl_float64(slope, offset, power, saturation, N):
    """The header's formula in float64: (the bytes as an (N, N, N, 3) array [blue][green][red], 255 w before rounding, y)."""
    x = np.arange(N, dtype=np.float64) / (N - 1)
    k, j, i = np.meshgrid(x, x, x, indexing="ij")
    y = [np.clip(c * s + o, 0.0, 1.0) for c, s, o in zip((i, j, k), slope, offset)]
    z = [np.where(v > 0.0, v, 0.0) ** p for v, p in zip(y, power)]
    luma = 0.2126 * z[0] + 0.7152 * z[1] + 0.0722 * z[2]
    w = np.stack([255.0 * np.clip(saturation * (c - luma) + luma, 0.0, 1.0) for c in z], axis=-1)
    return np.floor(w + 0.5).astype(np.int64), w, np.stack(y, axis=-1)


# Parameter sets whose lattice keeps every positive y at or above 0.001 and every power at or below 64: the range in which the devmath
# tests hold det_pow to a relative error of 1e-5 (tests/test_spot_lights.py test_det_pow_spot_range).
BUILDER_SETS = {
    "warm": dict(slope=(1.1, 1.0, 0.9), offset=(0.02, 0.0, -0.03125), power=(0.9, 1.0, 1.1), saturation=1.15),
    "grey": dict(slope=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), power=(1.0, 1.0, 1.0), saturation=0.0),
    "contrast": dict(slope=(1.3, 1.3, 1.3), offset=(-0.125, -0.125, -0.125), power=(1.5, 1.5, 1.5), saturation=0.8),
    "lifted": dict(slope=(0.8, 0.85, 0.9), offset=(0.05, 0.05, 0.06), power=(0.5, 0.6, 2.2), saturation=1.5),
}
DET_POW_REL = 1e-5


def _params(built_lib, p):
    return built_lib.GradeParams.default(**p)


def _build(built_lib, p, N):
    lut = np.zeros((N, N, N, 4), np.uint8)
    q = None if p is None else _params(built_lib, p)
    built_lib.check(built_lib.lib.crychic_grade_build_lut(None if q is None else C.byref(q), N, lut.ctypes.data, lut.nbytes))
    return lut


def test_builder_identity_is_the_identity_table(built_lib):
    for N in range(2, gl.MAX_N + 1):
        assert np.array_equal(_build(built_lib, None, N), gl.identity_lut(N)), N


def test_builder_host_body_equals_the_entry(built_lib):
    for name, p in BUILDER_SETS.items():
        flat = list(p["slope"]) + list(p["offset"]) + list(p["power"]) + [p["saturation"]]
        for N in (2, 17, 33):
            assert np.array_equal(gh.build_lut(flat, N), _build(built_lib, p, N)), (name, N)


@pytest.mark.parametrize("name", list(BUILDER_SETS))
def test_builder_against_float64(built_lib, name):
    """Every byte within 1 of the float64 restatement, and a byte differs only where the restatement's own 255 w lies within delta of
    a .5 tie.  delta is a condition worked out here, not a measurement: det_pow's bound, the binary32 roundings in front of it
    carried through the power's slope, the saturation's mix, times 255.  The share of such entries is capped at 4 delta -- twice
    what values spread evenly over a byte's width would give, because a lattice is not spread evenly -- and the parameter sets are
    chosen so that the restatement alone stays inside that cap."""
    p = BUILDER_SETS[name]
    lines = []
    for N in (17, 33):
        ref, w, y = cdl_float64(p["slope"], p["offset"], p["power"], p["saturation"], N)
        pos = y[y > 0.0]
        assert pos.min() >= 0.001 and max(p["power"]) <= 64.0, "the set leaves the range det_pow's bound is held in"
        e_y = (max(p["slope"]) + 2.0) * 2.0 ** -23                   # x, the product and the sum: one rounding each, of values <= slope + 1
        gain = max(float((pw * np.where(y[..., c] > 0, y[..., c], 1.0) ** (pw - 1.0)).max()) for c, pw in enumerate(p["power"]))
        e_z = DET_POW_REL + gain * e_y
        e_w = (2.0 * p["saturation"] + 1.0) * e_z + 4.0 * 2.0 ** -24
        delta = 255.0 * e_w + 2.0 ** -16                                 # and the last fma's rounding, of a value below 256
        cap = 4.0 * delta
        near = np.abs(w - np.floor(w) - 0.5) <= delta
        got = _build(built_lib, p, N)[..., :3].astype(np.int64)
        diff = got != ref
        share, near_share = float(diff.mean()), float(near.mean())
        lines.append("%s N=%d: delta %.3e, cap %.3e, entries within delta of a tie %.3e, bytes that differ %.3e (%d of %d), largest difference %d"
                     % (name, N, delta, cap, near_share, share, int(diff.sum()), diff.size, int(np.abs(got - ref).max())))
        print(lines[-1])
        assert np.abs(got - ref).max() <= 1
        assert near_share <= cap, "the parameter set itself crowds the ties: choose another"
        assert not (diff & ~near).any(), "a byte differs away from every tie"
        assert share <= cap
        assert (_build(built_lib, p, N)[..., 3] == 255).all()


def test_builder_black_stays_black(built_lib):
    lut = _build(built_lib, dict(power=(0.0625, 1.0, 16.0), saturation=1.0), 9)
    assert (lut[0, 0, 0, :3] == 0).all(), "y = 0 does not give 0"


def test_builder_refusals(built_lib):
    f = built_lib.lib.crychic_grade_build_lut
    buf = np.zeros(4 * 33 ** 3, np.uint8)
    assert f(None, 1, buf.ctypes.data, buf.nbytes) == -1 and f(None, 34, buf.ctypes.data, buf.nbytes) == -1
    assert f(None, 33, None, buf.nbytes) == -1
    assert f(None, 33, buf.ctypes.data, buf.nbytes - 1) == -1
    assert f(None, 33, buf.ctypes.data, buf.nbytes) == 0
    assert built_lib.lib.crychic_grade_default_params(None) == -1
    for field, bad in (("slope", -0.1), ("slope", 16.5), ("offset", -4.5), ("offset", 4.5), ("power", 0.0), ("power", 0.06), ("power", 17.0),
                       ("saturation", -0.1), ("saturation", 4.1)):
        for v in (bad, float("nan"), float("inf"), float("-inf")):
            q = built_lib.GradeParams.default()
            if field == "saturation":
                q.saturation = v
            else:
                getattr(q, field)[1] = v
            assert f(C.byref(q), 5, buf.ctypes.data, buf.nbytes) == -1, (field, v)
            assert field in built_lib.lib.crychic_last_error().decode()
    d = built_lib.GradeParams.default()
    assert list(d.slope) == [1.0] * 3 and list(d.offset) == [0.0] * 3 and list(d.power) == [1.0] * 3 and d.saturation == 1.0


# ---- the .cube loader ----------------------------------------------------------------------------------------------------------------

def load_cube(built_lib, path, capacity=None, want_table=True):
    buf = np.full(4 * gl.MAX_N ** 3 if capacity is None else capacity, gl.GUARD, np.uint8)
    n = C.c_uint32(0)
    rc = built_lib.lib.crychic_load_cube_lut(os.fsencode(str(path)), buf.ctypes.data if want_table else None, buf.nbytes, C.byref(n))
    N = int(n.value)
    return rc, N, (buf[:4 * N ** 3].reshape(N, N, N, 4) if rc == 0 and want_table else buf)


def test_cube_loader_reads_what_the_writer_wrote(built_lib, tmp_path):
    for N, newline in ((2, "\n"), (5, "\r\n"), (17, "\n"), (33, "\r\n")):
        lut = gl.corpus_lut(N).copy()
        lut[..., 3] = 255
        rc, n, got = load_cube(built_lib, gl.write_cube(tmp_path / ("t%d.cube" % N), lut, newline))
        assert rc == 0 and n == N and np.array_equal(got, lut), (N, newline)
    # the header in any order, with comments, blank lines, indentation and both domains; values outside 0 .. 1 clamp
    lut = gl.identity_lut(3)
    head = ["", "  # a comment", "DOMAIN_MAX 1.0 1.0 1.0", "LUT_3D_SIZE 3", "#another", 'TITLE "LUT_1D_SIZE 7 is only a title here"', "DOMAIN_MIN 0 0 0", "\t"]
    rc, n, got = load_cube(built_lib, gl.write_cube(tmp_path / "order.cube", lut, "\r\n", head))
    assert rc == 0 and n == 3 and np.array_equal(got, lut)
    p = tmp_path / "clamp.cube"
    p.write_text("LUT_3D_SIZE 2\n" + "-0.5 1.5 0.5\n" * 7 + "1e-3 2 0.5")          # the last line without a newline
    rc, n, got = load_cube(built_lib, p)
    assert rc == 0 and n == 2 and (got[0, 0, 0] == (0, 255, 128, 255)).all() and (got[1, 1, 1] == (0, 255, 128, 255)).all()
    # the size alone
    rc, n, buf = load_cube(built_lib, tmp_path / "t17.cube", want_table=False)
    assert rc == 0 and n == 17 and (buf == gl.GUARD).all()


def test_cube_loader_refusals(built_lib, tmp_path):
    rows2 = ["0 0 0"] * 8

    def refuse(name, lines, newline="\n", raw=None, capacity=None):
        p = tmp_path / (name + ".cube")
        p.write_bytes(raw if raw is not None else (newline.join(lines) + newline).encode())
        rc, _, _ = load_cube(built_lib, p, capacity)
        assert rc in (-1, -4), "%s: status %d" % (name, rc)
        return rc

    assert refuse("one_d", ["LUT_1D_SIZE 8"] + rows2) == -4
    assert refuse("domain_min", ["DOMAIN_MIN 0 0 0.1", "LUT_3D_SIZE 2"] + rows2) == -4
    assert refuse("domain_max", ["LUT_3D_SIZE 2", "DOMAIN_MAX 2 2 2"] + rows2) == -4
    assert refuse("n_1", ["LUT_3D_SIZE 1", "0 0 0"]) == -4
    assert refuse("n_34", ["LUT_3D_SIZE 34"] + ["0 0 0"] * 34 ** 3) == -4
    assert refuse("n_huge", ["LUT_3D_SIZE 4000000000"] + rows2) == -4
    assert refuse("n_fraction", ["LUT_3D_SIZE 2.5"] + rows2) == -4
    assert refuse("too_few", ["LUT_3D_SIZE 2"] + rows2[:7]) == -1
    assert refuse("too_many", ["LUT_3D_SIZE 2"] + rows2 + ["0 0 0"]) == -1
    assert refuse("no_size", rows2) == -1
    assert refuse("two_sizes", ["LUT_3D_SIZE 2", "LUT_3D_SIZE 2"] + rows2) == -1
    assert refuse("late_keyword", ["LUT_3D_SIZE 2"] + rows2[:3] + ["TITLE late"] + rows2[3:]) == -1
    assert refuse("unparsable", ["LUT_3D_SIZE 2"] + rows2[:7] + ["0 0 0x"]) == -1
    assert refuse("two_numbers", ["LUT_3D_SIZE 2"] + rows2[:7] + ["0 0"]) == -1
    assert refuse("four_numbers", ["LUT_3D_SIZE 2"] + rows2[:7] + ["0 0 0 0"]) == -1
    assert refuse("overflow", ["LUT_3D_SIZE 2"] + rows2[:7] + ["0 1e999 0"]) == -1
    assert refuse("minus_nan", ["LUT_3D_SIZE 2"] + rows2[:7] + ["0 -nan 0"]) == -1
    refuse("nan", ["LUT_3D_SIZE 2"] + rows2[:7] + ["nan 0 0"])
    refuse("inf", ["LUT_3D_SIZE 2"] + ["inf 0 0"] + rows2[:7])
    assert refuse("long_line", ["LUT_3D_SIZE 2", "#" + "x" * 1024] + rows2) == -1
    assert refuse("capacity", ["LUT_3D_SIZE 2"] + rows2, capacity=31) == -1
    assert refuse("garbage", None, raw=bytes(np.random.default_rng(3).integers(0, 256, 4096, dtype=np.uint8))) < 0
    assert refuse("nul", None, raw=b"LUT_3D_SIZE 2\n0 0 \x000\n" + b"0 0 0\n" * 7) == -1
    assert refuse("empty", None, raw=b"") == -1
    f = built_lib.lib.crychic_load_cube_lut
    n = C.c_uint32()
    buf = np.zeros(64, np.uint8)
    assert f(None, buf.ctypes.data, 64, C.byref(n)) == -1
    assert f(os.fsencode(str(tmp_path / "missing.cube")), buf.ctypes.data, 64, C.byref(n)) == -1
    assert f(os.fsencode(str(tmp_path / "capacity.cube")), buf.ctypes.data, 64, None) == -1
    # the line of 1023 bytes is a line
    p = tmp_path / "fits.cube"
    p.write_text("LUT_3D_SIZE 2\n#" + "x" * 1022 + "\n" + "0 0 0\n" * 8)
    assert load_cube(built_lib, p)[0] == 0
