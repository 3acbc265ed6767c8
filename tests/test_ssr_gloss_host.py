"""crychic_ssr_pyramid and crychic_ssr_glossy on the CPU tier: the kernel bodies (csrc/ssr_pyramid_core.hpp and csrc/ssr_gloss_core.hpp,
built for the host with the workgroup and lane walks emulated) against the checker (tests/ssr_gloss_ref, plain C from the definition in
include/crychic_hip.h), byte for byte on the pyramid's sizes and on ssr_lib's corpus under three gloss settings, behind guard bytes
and on misaligned planes; the branches the corpus must reach; the definition's known answers and its level anchor; row ranges; and the
refusals of the real library, which need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import ssr_gloss_host_lib as host
import ssr_gloss_lib as gl
import ssr_lib as sl


@pytest.fixture(scope="module")
def cases(built_lib):
    return sl.corpus()


def host_pyramid(img, levels, misalign=0):
    """The kernel body's pyramid of `img`, the frame `misalign` bytes past a 64-byte boundary, in a guarded 16-byte aligned workspace
    of GUARD: a flat uint8 array as gl.pyramid gives it; asserts the guard bytes and that the frame did not change."""
    H, W = img.shape[:2]
    sraw, src = sl.guarded(img.shape, misalign=misalign)
    src[...] = img
    wraw, ws = sl.guarded((max(gl.plan(W, H, levels)[2], 16),))
    groups = host.pyramid(src, levels, ws)
    assert sl.guards_intact(sraw, src) and sl.guards_intact(wraw, ws), "guard bytes changed"
    assert np.array_equal(src, img), "the frame changed"
    assert (groups == 0) == (gl.plan(W, H, levels)[0] == 0)
    return ws


def run_host(frame, img, params=None, gloss=None, row0=0, rows=None, mix=0, misalign=0, pyr=None):
    """The kernel bodies -- the pyramid's, unless `pyr` is given, then the pass's -- on guarded copies of `img`, `misalign` bytes past a
    64-byte boundary: the output plane; asserts the guard bytes and that nothing but `out` changed."""
    levels = int(gl.gloss_array(gloss)[1])
    pyr = host_pyramid(img, levels, misalign) if pyr is None else pyr
    sraw, src = sl.guarded(img.shape, misalign=misalign)
    oraw, out = sl.guarded(img.shape, misalign=misalign)
    praw, p = sl.guarded(pyr.shape)
    src[...] = img
    p[...] = pyr
    host.glossy(frame, src, p, out, params, gloss, row0, rows, mix=mix)
    assert sl.guards_intact(sraw, src) and sl.guards_intact(oraw, out) and sl.guards_intact(praw, p), "guard bytes changed"
    assert np.array_equal(src, img) and np.array_equal(p, pyr), "an input plane changed"
    return out


# ---- the pyramid alone --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", gl.PYRAMID_SIZES, ids=lambda s: "%dx%d" % s)
def test_pyramid_host_body_equals_checker(built_lib, size):
    W, H = size
    img = gl.pyramid_frame(W, H)
    for levels in (8, 3, 1):
        ref = gl.pyramid(img, levels)
        n, sizes, nbytes = gl.plan(W, H, levels)
        assert n <= levels - 1 and (n == levels - 1 or sizes[n][:2] == (1, 1))
        assert nbytes == built_lib.lib.crychic_ssr_pyramid_bytes(W, H, levels)
        assert [s[2] for s in sizes[1:]] == [built_lib.lib.crychic_ssr_pyramid_offset(W, H, levels, k) for k in range(1, n + 1)]
        assert all(o % 16 == 0 for _, _, o in sizes) and built_lib.lib.crychic_ssr_pyramid_offset(W, H, levels, n + 1) == 0
        for misalign in (0, 4, 12):
            got = host_pyramid(img, levels, misalign)
            assert np.array_equal(got, ref), "%dx%d, %d levels, the frame %d bytes past a 64-byte boundary" % (W, H, levels, misalign)
    assert built_lib.lib.crychic_ssr_pyramid_bytes(W, H, 0) == 0 and built_lib.lib.crychic_ssr_pyramid_bytes(W, H, 9) == 0
    assert built_lib.lib.crychic_ssr_pyramid_bytes(0, H, 6) == 0 and built_lib.lib.crychic_ssr_pyramid_bytes(W, 0, 6) == 0


def test_pyramid_level_sizes():
    n, sizes, nbytes = gl.plan(130, 70, 8)
    assert n == 7 and [s[:2] for s in sizes] == [(130, 70), (65, 35), (33, 18), (17, 9), (9, 5), (5, 3), (3, 2), (2, 1)]
    assert gl.plan(130, 70, 1) == (0, [(130, 70, 0)], 0) and gl.plan(1, 1, 8)[0] == 0 and gl.plan(2, 2, 8)[0] == 1 and gl.plan(1, 7, 8)[0] == 3


def test_pyramid_known_answers(built_lib):
    gl.check_pyramid_answers(lambda img, levels: gl.level_views(gl.pyramid(img, levels), img.shape[1], img.shape[0], levels))
    gl.check_pyramid_answers(lambda img, levels: gl.level_views(host_pyramid(img, levels), img.shape[1], img.shape[0], levels))


# ---- the pass -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gname", list(gl.GLOSS_SETS))
@pytest.mark.parametrize("pname", list(sl.PARAM_SETS))
def test_host_body_equals_checker(cases, pname, gname):
    ran = 0
    for name, frame, img, pn, mix in cases:
        if pn != pname:
            continue
        pyr, ref, _, _ = gl.expected(name, gname)
        for misalign in (0, 4, 12):
            hp = host_pyramid(img, gl.GLOSS_SETS[gname]["levels"], misalign)
            assert np.array_equal(hp, pyr), "%s: the pyramid differs" % name
            got = run_host(frame, img, sl.PARAM_SETS[pn], gl.GLOSS_SETS[gname], mix=mix, misalign=misalign, pyr=hp)
            assert np.array_equal(got, ref), "%s under %s, planes %d bytes past a 64-byte boundary: %d bytes differ" % (
                name, gname, misalign, int((got != ref).sum()))
        ran += 1
    assert ran >= 6


def test_the_corpus_reaches_every_branch(cases):
    """With the checker alone: over the corpus under the three settings every branch of 6a and 6b is taken, and the debug plane's
    first four words are crychic_ssr's (steps 1 to 6 stand)."""
    total = dict.fromkeys(gl.COUNTERS, 0)
    for name, frame, img, pname, _ in cases:
        _, n0, dbg0 = sl.expected(name)
        for gname in gl.GLOSS_SETS:
            _, _, n, dbg = gl.expected(name, gname)
            for k in total:
                total[k] += n[k]
            assert all(n[k] == n0[k] for k in sl.COUNTERS), name
            assert n["lq_zero"] + n["lq_positive"] == n["hit_first"] + n["hit_later"] == n["f_zero"] + n["f_positive"], name
            assert np.array_equal(dbg[..., :4], dbg0), name
            hit = dbg[..., 0] == sl.ST_HIT
            n_eff = gl.plan(img.shape[1], img.shape[0], gl.GLOSS_SETS[gname]["levels"])[0]
            assert (dbg[..., 4][hit] >= 0).all() and (dbg[..., 4][hit] <= 256 * n_eff).all(), name
    assert all(total[k] > 0 for k in gl.BRANCHES), total


def glossy_answers(fn):
    """The definition's known answers for fn(frame, img, params, gloss) -> the frame behind the pass."""
    rng = np.random.default_rng(11)
    sc = sl.scene_frame()
    img = rng.integers(0, 256, (96, 128, 4), dtype=np.uint8)
    sharp, n, _ = sl.checker(sc, img, sl.PARAM_SETS["mirror_n64"])
    assert n["hit_first"] + n["hit_later"] > 0
    wide = dict(coneScale=16.0, levels=8)
    blurred = fn(sc, img, sl.PARAM_SETS["mirror_n64"], wide)
    assert not np.array_equal(blurred, sharp), "the cone changes nothing"
    assert np.array_equal(blurred[..., 3], img[..., 3]), "alpha is the pixel's own"
    # coneScale 0, one level, or roughness 0 everywhere: crychic_ssr's bytes
    for pname in ("default", "mirror_n64", "thick_n2"):
        ref, _, _ = sl.checker(sc, img, sl.PARAM_SETS[pname])
        assert np.array_equal(fn(sc, img, sl.PARAM_SETS[pname], dict(coneScale=0.0, levels=8)), ref), pname
        assert np.array_equal(fn(sc, img, sl.PARAM_SETS[pname], dict(coneScale=16.0, levels=1)), ref), pname
    g1 = sc.g[1].copy()
    g1[..., 3] = 0.0
    smooth = sc.with_(g1=g1)
    ref, n, _ = sl.checker(smooth, img, sl.PARAM_SETS["mirror_n64"])
    assert n["hit_first"] + n["hit_later"] > 0 and np.array_equal(fn(smooth, img, sl.PARAM_SETS["mirror_n64"], wide), ref)
    # a frame of one colour stays that colour under any G-buffer, depth and parameters
    one = np.empty((96, 128, 4), np.uint8)
    one[...] = (200, 3, 97, 41)
    wild = sc.with_(depth=sl.make_depth("random", 128, 96, rng), **dict(zip(("g0", "g1", "g2"), sl.random_gbuffer(128, 96, rng))))
    for f in (sc, wild):
        for gname in gl.GLOSS_SETS:
            assert np.array_equal(fn(f, one, sl.PARAM_SETS["thick_n2"], gl.GLOSS_SETS[gname]), one), gname


def test_known_answers(built_lib):
    glossy_answers(lambda f, i, p, g: gl.checker(f, i, p, g)[0])
    glossy_answers(lambda f, i, p, g: run_host(f, i, p, g))


@pytest.mark.parametrize("size", [(128, 96), (70, 38)])
def test_level_anchor(built_lib, size):
    """The mirror scene with a floor of roughness 0.5: the level the pass picks follows the float64 screen length of the true
    reflected ray (ssr_gloss_lib.check_level_anchor) -- and the host body writes the same frame."""
    W, H = size
    frame, img, truth = gl.anchor_scene(W, H)
    out, n, dbg = gl.checker(frame, img, sl.PARAM_SETS["mirror_n64"], gl.ANCHOR_GLOSS)
    gl.check_level_anchor(W, H, dbg, truth)
    assert np.array_equal(run_host(frame, img, sl.PARAM_SETS["mirror_n64"], gl.ANCHOR_GLOSS), out)


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 190), (0, 7, 12, 95, 190)])
def test_row_ranges_stitch_to_the_whole_frame(cases, split):
    by_name = {c[0]: c for c in cases}
    for name, gname in (("322x190_ramp_long_n63", "c16_l8"), ("322x190_zeros_mirror_n64", "default")):
        _, frame, img, pname, _ = by_name[name]
        pyr, whole, _, _ = gl.expected(name, gname)
        stitched = np.full(img.shape, sl.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got = run_host(frame, img, sl.PARAM_SETS[pname], gl.GLOSS_SETS[gname], row0=row0, rows=end - row0, pyr=pyr)
            assert (got[:row0] == sl.GUARD).all() and (got[end:] == sl.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
        assert np.array_equal(stitched, whole), name


def test_default_params(built_lib):
    p = built_lib.SsrGlossParams()
    assert C.sizeof(p) == 16 and built_lib.lib.crychic_ssr_gloss_default_params(C.byref(p)) == 0
    assert (p.coneScale, p.levels, tuple(p.reserved)) == (np.float32(gl.GLOSS_DEFAULTS["coneScale"]), gl.GLOSS_DEFAULTS["levels"], (0, 0))
    assert built_lib.lib.crychic_ssr_gloss_default_params(None) == -1 and built_lib.SSR_GLOSS_MAX_LEVELS == gl.MAX_LEVELS == 8
    q = built_lib.SsrGlossParams.default(coneScale=1.25, levels=3)
    assert (q.coneScale, q.levels) == (1.25, 3)


def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, G = built_lib.lib, built_lib.SsrGlossParams
    a, b, d, w = 0x10000000, 0x20000000, 0x30000000, 0x70000000           # never dereferenced
    g = [0x40000000, 0x50000000, 0x60000000]
    good = sl.camera_constants(64, 32)
    need = lib.crychic_ssr_pyramid_bytes(64, 32, 6)
    ok = (-1, "null context")

    def glossy(src=a, pyr=w, nbytes=need, dst=b, W=64, H=32, row0=0, rows=32, flags=0, params=None, gloss=None, planes=g):
        rc = lib.crychic_ssr_glossy(None, C.byref(good), planes[0], planes[1], planes[2], d, src, pyr, nbytes, dst, W, H, row0, rows, flags,
                                    None if params is None else C.byref(params), None if gloss is None else C.byref(gloss), None)
        return rc, lib.crychic_last_error().decode()

    def pyramid(src=a, W=64, H=32, levels=6, ws=w, nbytes=need):
        return lib.crychic_ssr_pyramid(None, src, W, H, levels, ws, nbytes, None), lib.crychic_last_error().decode()

    def gp(**kw):
        return G.default(**kw)
    assert glossy() == ok and pyramid() == ok
    assert glossy(gloss=gp(coneScale=0.0, levels=1), pyr=None, nbytes=0) == ok, "one level needs no pyramid"
    assert glossy(gloss=gp(coneScale=16.0, levels=8), nbytes=lib.crychic_ssr_pyramid_bytes(64, 32, 8)) == ok
    assert pyramid(levels=1, ws=None, nbytes=0) == ok and pyramid(W=1, H=1, levels=8, ws=None, nbytes=0) == ok
    assert pyramid(ws=a + 64 * 32 * 4) == ok, "adjacent ranges do not overlap"
    assert pyramid(W=1 << 22, H=64, levels=2, nbytes=1 << 28) == ok                                      # 2^28 pixels
    for kw, word in ((dict(src=None), "null argument"), (dict(ws=None), "null argument"), (dict(src=a + 2), "aligned"), (dict(ws=w + 8), "16-byte aligned"),
                     (dict(W=0), "non-zero"), (dict(H=0), "non-zero"), (dict(levels=0), "levels"), (dict(levels=9), "levels"),
                     (dict(nbytes=need - 1), "needs"), (dict(levels=8), "needs"), (dict(ws=a), "overlaps"), (dict(ws=a + 64 * 32 * 4 - 16), "overlaps"),
                     (dict(src=w + need - 4), "overlaps")):
        rc, msg = pyramid(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = pyramid(W=1 << 15, H=(1 << 13) + 1, nbytes=1 << 30)
    assert rc == -4 and "exceeds" in msg
    bad_res = gp()
    bad_res.reserved[1] = 1
    for kw, word in ((dict(src=None), "null argument"), (dict(dst=None), "null argument"), (dict(pyr=None), "null argument"),
                     (dict(planes=[g[0], None, g[2]]), "null argument"), (dict(pyr=w + 4), "16-byte aligned"), (dict(src=a + 2), "aligned"),
                     (dict(row0=1, rows=32), "outside the 32-row frame"), (dict(flags=1), "flags"),
                     (dict(params=built_lib.SsrParams.default(steps=65)), "steps"), (dict(dst=a), "overlap"),
                     (dict(gloss=gp(coneScale=-0.5)), "coneScale"), (dict(gloss=gp(coneScale=16.5)), "coneScale"),
                     (dict(gloss=gp(coneScale=math.nan)), "coneScale"), (dict(gloss=gp(coneScale=math.inf)), "coneScale"),
                     (dict(gloss=gp(levels=0)), "levels"), (dict(gloss=gp(levels=9)), "levels"), (dict(gloss=bad_res), "reserved"),
                     (dict(nbytes=need - 1), "needs"), (dict(gloss=gp(levels=7)), "needs"), (dict(pyr=b), "overlaps"),
                     (dict(pyr=b + 64 * 32 * 4 - 16), "overlaps")):
        rc, msg = glossy(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
