"""crychic_ssr on the CPU tier: the kernel body (csrc/ssr_core.hpp, built for the host with the workgroup and lane walk emulated)
against the checker (tests/ssr_ref, plain C from the definition in include/crychic_hip.h), byte for byte on the whole corpus, behind
guard bytes and on misaligned planes; what the corpus must reach, checked with the checker alone; the definition's known answers and
its mirror anchor; row ranges; and the refusals of the real library, which need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import ssr_host_lib as host
import ssr_lib as sl


@pytest.fixture(scope="module")
def cases(built_lib):
    return sl.corpus()


def run_host(frame, img, params=None, row0=0, rows=None, mix=0, misalign=0):
    """The kernel body on guarded copies of `img`, the depth plane and the G-buffer planes in the formats of `mix`, `misalign` bytes
    (a multiple of 4; the G-buffer planes: of their texel) past a 64-byte boundary: the output plane; asserts the guard bytes around
    the planes and that nothing but `out` changed."""
    sraw, src = sl.guarded(img.shape, misalign=misalign)
    draw, depth = sl.guarded(frame.depth.shape, np.uint32, misalign=misalign)
    oraw, out = sl.guarded(img.shape, misalign=misalign)
    src[...] = img
    depth[...] = frame.depth
    planes, raws = [], []
    for k in range(3):
        p = frame.plane(k, mix)
        raw, view = sl.guarded(p.shape, p.dtype, misalign=p.dtype.itemsize * 4 if misalign else 0)       # one texel
        view[...] = p
        planes.append(view)
        raws.append(raw)
    host.ssr(frame, src, out, params, row0, rows, mix=mix, planes=planes, depth=depth)
    assert sl.guards_intact(sraw, src) and sl.guards_intact(oraw, out) and sl.guards_intact(draw, depth), "guard bytes changed"
    assert all(sl.guards_intact(r, v) for r, v in zip(raws, planes)), "guard bytes of a G-buffer plane changed"
    assert np.array_equal(depth, frame.depth) and np.array_equal(src, img), "an input plane changed"
    assert all(np.array_equal(v.view(np.uint8), frame.plane(k, mix).view(np.uint8)) for k, v in enumerate(planes)), "a G-buffer plane changed"
    return out


@pytest.mark.parametrize("pname", list(sl.PARAM_SETS))
def test_host_body_equals_checker(cases, pname):
    ran = 0
    for name, frame, img, pn, mix in cases:
        if pn != pname:
            continue
        ref, _, _ = sl.expected(name)
        for misalign in (0, 4, 12):
            got = run_host(frame, img, sl.PARAM_SETS[pn], mix=mix, misalign=misalign)
            assert np.array_equal(got, ref), "%s, planes %d bytes past a 64-byte boundary: %d bytes differ" % (name, misalign, int((got != ref).sum()))
        ran += 1
    assert ran >= 6


def test_the_corpus_reaches_what_it_must(cases):
    """With the checker alone: every size, N, depth kind and format mix is there; every branch the checker counts is taken; an 8 x 8
    tile of one wavefront holds both marching and exiting lanes; rays cross workgroup rows."""
    assert {img.shape[1::-1] for _, _, img, _, _ in cases} >= set(sl.SIZES) | {(64, 64), (128, 96), (70, 38), (4100, 3), (3, 4100)}
    assert {sl.PARAM_SETS[p]["steps"] for _, _, _, p, _ in cases} == {1, 2, 32, 63, 64}
    assert {p for _, _, _, p, _ in cases} == set(sl.PARAM_SETS) and len(sl.PARAM_SETS) == 5
    assert {m for _, _, _, _, m in cases} == set(range(8))
    total = dict.fromkeys(sl.COUNTERS, 0)
    mixed_tiles = crossing = 0
    for name, frame, img, pname, _ in cases:
        _, n, dbg = sl.expected(name)
        H, W = img.shape[:2]
        hits = n["hit_first"] + n["hit_later"]
        assert n["sky"] + n["rough"] + n["behind_near"] + n["no_hit"] + hits == W * H, name
        assert n["left_frame"] + n["past_far"] <= n["no_hit"], name
        for k in total:
            total[k] += n[k]
        st = dbg[..., 0]
        assert (st >= 0).all() and int((st == sl.ST_HIT).sum()) == hits, name
        marching = st >= sl.ST_LEFT_FRAME               # the lane went into the march
        for y in range(0, H, 8):
            for x in range(0, W, 8):
                t = marching[y:y + 8, x:x + 8]
                mixed_tiles += bool(t.any() and not t.all())
        ys = np.nonzero(st == sl.ST_HIT)[0]
        crossing += int((dbg[..., 2][st == sl.ST_HIT] // 8 != ys // 8).sum())
    assert all(v > 0 for v in total.values()), total
    assert mixed_tiles > 0, "no wavefront with both marching and exiting lanes"
    assert crossing > 0, "no ray crosses a workgroup row"
    for name in ("vp_inf", "vp_nan", "vp_w_inf"):
        assert not np.isfinite({c[0]: c for c in cases}[name][1].vp).all()
    nf = {c[0]: c for c in cases}["gbuffer_nonfinite"][1]
    assert all(np.isnan(g).any() and np.isinf(g).any() for g in nf.g)
    assert (np.abs({c[0]: c for c in cases}["normals_zero"][1].g[2][..., :3]).sum(-1) == 0).any()


def answers(fn):
    """The definition's known answers for fn(frame, img, params) -> the frame behind the pass."""
    rng = np.random.default_rng(9)
    sc = sl.scene_frame()
    img = rng.integers(0, 256, (96, 128, 4), dtype=np.uint8)
    changed = fn(sc, img, sl.DEFAULTS)
    assert not np.array_equal(changed, img), "the scene reflects nothing"
    assert np.array_equal(changed[..., 3], img[..., 3]), "alpha is the pixel's own"
    # maxRoughness 0, intensity 0, a depth plane of sky: out == in
    for N in (1, 32, 64):
        assert np.array_equal(fn(sc, img, dict(sl.DEFAULTS, maxRoughness=0.0, steps=N)), img)
        assert np.array_equal(fn(sc, img, dict(sl.DEFAULTS, intensity=0, steps=N)), img)
    assert np.array_equal(fn(sc.with_(depth=sl.make_depth("ones", 128, 96, rng)), img, sl.DEFAULTS), img)
    # a frame of one colour stays that colour under any G-buffer, depth and parameters
    one = np.empty((96, 128, 4), np.uint8)
    one[...] = (200, 3, 97, 41)
    wild = sc.with_(depth=sl.make_depth("random", 128, 96, rng), **dict(zip(("g0", "g1", "g2"), sl.random_gbuffer(128, 96, rng))))
    for f in (sc, wild):
        for pname in sl.PARAM_SETS:
            assert np.array_equal(fn(f, one, sl.PARAM_SETS[pname]), one), pname
    # a pixel the pass does not touch keeps its bytes: whatever does not reflect, and whatever has no hit
    out, _, dbg = sl.checker(wild, img, sl.PARAM_SETS["thick_n2"])
    got = fn(wild, img, sl.PARAM_SETS["thick_n2"])
    untouched = dbg[..., 0] != sl.ST_HIT
    assert untouched.any() and np.array_equal(got[untouched], img[untouched]) and np.array_equal(got, out)


def test_known_answers(built_lib):
    answers(lambda f, i, p: sl.checker(f, i, p)[0])
    answers(lambda f, i, p: run_host(f, i, p))


@pytest.mark.parametrize("size", [(128, 96), (70, 38)])
def test_mirror_anchor(built_lib, size):
    """A mirror floor in front of a wall whose colour encodes its pixel: the checker's hit pixel lies within 1 + stride / 16 pixels of
    the projection of the point where the float64 mirrored ray meets the wall, at least 90 % of the eligible pixels report a hit,
    the colour is the blend with that texel -- and the host body writes the same frame."""
    W, H = size
    frame, img, truth = sl.mirror_scene(W, H)
    out, n, dbg = sl.checker(frame, img, sl.PARAM_SETS["mirror_n64"])
    sl.check_mirror(W, H, out, dbg, frame, img, truth)
    assert np.array_equal(run_host(frame, img, sl.PARAM_SETS["mirror_n64"]), out)


SPLITS = [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 190)]       # the fog's


@pytest.mark.parametrize("split", SPLITS)
def test_row_ranges_stitch_to_the_whole_frame(cases, split):
    by_name = {c[0]: c for c in cases}
    leaving = 0
    for name in ("322x190_ramp_long_n63", "322x190_zeros_mirror_n64"):
        _, frame, img, pname, _ = by_name[name]
        whole, _, dbg = sl.expected(name)
        stitched = np.full(img.shape, sl.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got = run_host(frame, img, sl.PARAM_SETS[pname], row0=row0, rows=end - row0)
            ref, _, _ = sl.checker(frame, img, sl.PARAM_SETS[pname], row0=row0, rows=end - row0)
            assert np.array_equal(got, ref), (name, row0, end)
            assert (got[:row0] == sl.GUARD).all() and (got[end:] == sl.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
            part = dbg[row0:end]
            hy = part[..., 2][part[..., 0] == sl.ST_HIT]
            leaving += int(((hy < row0) | (hy >= end)).sum())
        assert np.array_equal(stitched, whole), name
    assert leaving > 0, "no ray leaves the rows of its call"


def test_a_call_reads_the_frame_not_its_rows(cases):
    """Rows outside the call's range are read: changing them changes the range's result where a ray lands in them."""
    _, frame, img, pname, _ = {c[0]: c for c in cases}["322x190_ramp_long_n63"]
    whole, _, dbg = sl.expected("322x190_ramp_long_n63")
    part = dbg[120:160]
    hy = part[..., 2][part[..., 0] == sl.ST_HIT]
    assert ((hy < 120) | (hy >= 160)).any(), "no ray of these rows lands outside them"
    other = np.array(img)
    other[:120] ^= 0xFF
    other[160:] ^= 0xFF
    got = run_host(frame, other, sl.PARAM_SETS[pname], row0=120, rows=40)
    ref, _, _ = sl.checker(frame, other, sl.PARAM_SETS[pname], row0=120, rows=40)
    assert np.array_equal(got, ref) and not np.array_equal(got[120:160], whole[120:160])


def test_default_params(built_lib):
    p = built_lib.SsrParams()
    assert C.sizeof(p) == 32 and built_lib.lib.crychic_ssr_default_params(C.byref(p)) == 0
    assert (p.maxDistance, p.thickness, p.bias, p.maxRoughness) == (20.0, 0.5, np.float32(0.02), 0.75)
    assert (p.steps, p.edgeFade, p.intensity, p.reserved) == (32, 32, 256, 0)
    assert built_lib.lib.crychic_ssr_default_params(None) == -1
    assert built_lib.SSR_MAX_STEPS == 64
    q = built_lib.SsrParams.default(maxDistance=7.5, steps=3, intensity=9)
    assert (q.maxDistance, q.steps, q.intensity, q.thickness) == (7.5, 3, 9, 0.5)
    assert {k: getattr(p, k) for k in sl.DEFAULTS} == {k: (np.float32(v) if isinstance(v, float) else v) for k, v in sl.DEFAULTS.items()}


def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, P = built_lib.lib, built_lib.SsrParams
    a, b, d = 0x10000000, 0x20000000, 0x30000000           # never dereferenced
    g = [0x40000000, 0x50000000, 0x60000000]
    good = sl.camera_constants(64, 32)

    def call(cb=good, planes=g, depth=d, src=a, dst=b, W=64, H=32, row0=0, rows=32, flags=0, params=None):
        rc = lib.crychic_ssr(None, None if cb is None else C.byref(cb), planes[0], planes[1], planes[2], depth, src, dst, W, H, row0, rows, flags,
                             None if params is None else C.byref(params), None)
        return rc, lib.crychic_last_error().decode()

    def prm(**kw):
        return P.default(**kw)

    def cb_with(**proj):
        cb = built_lib.PassConstants.from_buffer_copy(good)
        for k, v in proj.items():
            cb.Proj[int(k[1:])] = v
        return cb
    ok = (-1, "null context")
    assert call() == ok
    assert call(dst=a + 64 * 32 * 4) == ok, "adjacent planes do not overlap"
    assert call(row0=32, rows=0) == ok and call(W=1, H=1, rows=1) == ok
    assert call(flags=0x7000, planes=[g[0] + 8, g[1] + 8, g[2] + 8]) == ok, "a half4 plane is 8-byte aligned"
    assert call(params=prm(steps=1, edgeFade=1, intensity=0, maxRoughness=0.0, bias=0.0)) == ok
    assert call(params=prm(steps=64, edgeFade=1024, maxRoughness=1.0, maxDistance=3e38, thickness=3e38)) == ok
    assert call(W=1 << 22, H=64, rows=1, dst=a + (1 << 30)) == ok and call(W=64, H=1 << 22, rows=1, dst=a + (1 << 30)) == ok      # 2^28 pixels, 2^22 columns or rows
    bad_res = prm()
    bad_res.reserved = 1
    for kw, word in ((dict(cb=None), "null argument"), (dict(depth=None), "null argument"), (dict(src=None), "null argument"), (dict(dst=None), "null argument"),
                     (dict(planes=[None, g[1], g[2]]), "null argument"), (dict(planes=[g[0], None, g[2]]), "null argument"),
                     (dict(planes=[g[0], g[1], None]), "null argument"),
                     (dict(src=a + 2), "aligned"), (dict(dst=b + 1), "aligned"), (dict(depth=d + 2), "aligned"),
                     (dict(planes=[g[0] + 8, g[1], g[2]]), "aligned"), (dict(planes=[g[0], g[1] + 4, g[2]]), "aligned"),
                     (dict(planes=[g[0], g[1], g[2] + 4], flags=0x4000), "aligned"),
                     (dict(W=0), "non-zero"), (dict(H=0, rows=0), "non-zero"),
                     (dict(row0=33, rows=0), "outside the 32-row frame"), (dict(row0=1, rows=32), "outside the 32-row frame"),
                     (dict(row0=0xFFFFFFFF, rows=2), "outside the 32-row frame"),
                     (dict(flags=1), "flags"), (dict(flags=0x8000), "flags"), (dict(flags=0x7001), "flags"),
                     (dict(params=prm(maxDistance=0.0)), "maxDistance"), (dict(params=prm(maxDistance=-1.0)), "maxDistance"),
                     (dict(params=prm(maxDistance=math.inf)), "maxDistance"), (dict(params=prm(maxDistance=math.nan)), "maxDistance"),
                     (dict(params=prm(thickness=0.0)), "thickness"), (dict(params=prm(thickness=math.inf)), "thickness"),
                     (dict(params=prm(thickness=math.nan)), "thickness"),
                     (dict(params=prm(bias=-0.1)), "bias"), (dict(params=prm(bias=0.5)), "bias"), (dict(params=prm(bias=math.nan)), "bias"),
                     (dict(params=prm(maxRoughness=-0.1)), "maxRoughness"), (dict(params=prm(maxRoughness=1.5)), "maxRoughness"),
                     (dict(params=prm(maxRoughness=math.nan)), "maxRoughness"),
                     (dict(params=prm(steps=0)), "steps"), (dict(params=prm(steps=65)), "steps"),
                     (dict(params=prm(edgeFade=0)), "edgeFade"), (dict(params=prm(edgeFade=1025)), "edgeFade"),
                     (dict(params=prm(intensity=257)), "intensity"), (dict(params=bad_res), "reserved"),
                     (dict(cb=cb_with(p10=math.nan)), "Proj[10]"), (dict(cb=cb_with(p10=math.inf)), "Proj[10]"),
                     (dict(cb=cb_with(p11=0.0)), "Proj[11]"), (dict(cb=cb_with(p11=-math.inf)), "Proj[11]"),
                     (dict(dst=a), "overlap"), (dict(dst=a + 4), "overlap"), (dict(dst=a + 64 * 32 * 4 - 4), "overlap"),
                     (dict(src=b + 64 * 32 * 4 - 4), "overlap")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    for kw in (dict(W=1 << 15, H=(1 << 13) + 1, rows=1), dict(W=(1 << 22) + 1, H=1, rows=1), dict(W=1, H=(1 << 22) + 1, rows=1)):
        rc, msg = call(**kw)
        assert rc == -4 and "exceeds" in msg, (kw, rc, msg)
