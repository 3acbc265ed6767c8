"""crychic_apply_decals on the CPU: the kernel body built for the host (tests/decal_host: the wavefront's box reduction, lane k's test
of decal k, the vote and the mask walk emulated) against the checker (tests/decal_ref: plain C from the header's text, every decal for
every pixel) byte for byte over the corpus; the tile masks against step 2; known answers against numpy; row ranges; every refusal;
crychic_decal_from_box."""
import ctypes as C

import numpy as np
import pytest

import decal_lib as dl
import decal_host_lib as dh


@pytest.fixture(scope="module")
def lib(built_lib):
    dl.build()
    dh.build()
    return built_lib


def host_run(frame, mix, decals, textures, ranges=None, misalign=0, masks=False):
    """The host body over each (row0, rows) of `ranges` on guarded copies of the frame's planes; the planes, the guards checked."""
    src = frame.planes(mix)
    g = [dl.guarded(p.shape, misalign=misalign) for p in src]
    for (raw, view), p in zip(g, src):
        view[...] = p
    planes = [view for _, view in g]
    m = None
    for row0, rows in (ranges or [(0, frame.H)]):
        r = dh.apply(frame, mix, decals, textures, planes, row0, rows, masks=masks)
        m = r[1] if masks else None
    assert all(dl.guards_intact(raw, view) for raw, view in g), "guard bytes changed"
    return (planes, m) if masks else planes


def assert_planes_equal(got, want, name):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "%s: G%d differs in %d bytes" % (name, k, int((a != b).sum()))


def test_checker_half_conversions_are_numpys(lib):
    ref = dl._ref()
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint32).view(np.float32), rng.normal(size=100000).astype(np.float32) * 1e-5,
                        rng.normal(size=100000).astype(np.float32) * 7e4,
                        np.array([0.0, -0.0, 65504.0, 65519.99, 65520.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -14, np.inf, -np.inf], np.float32)])
    x = x[~np.isnan(x)]
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    got = np.array([ref.decal_ref_f2h(float(v)) for v in x[:60000]] + [ref.decal_ref_f2h(float(v)) for v in x[-11:]], np.uint16)
    assert np.array_equal(got, np.concatenate([want[:60000], want[-11:]]))
    h = np.arange(65536, dtype=np.uint16)
    back = np.array([ref.decal_ref_h2f(int(v)) for v in h], np.float32)
    assert np.array_equal(back.view(np.uint32)[~np.isnan(back)], h.view(np.float16).astype(np.float32).view(np.uint32)[~np.isnan(back)])


def test_every_counter_of_the_checker_is_met(lib):
    tot = dl.total_counters()
    assert not [k for k, v in tot.items() if v == 0], tot


def test_scene_boxes_cover_what_the_issue_counted(lib):
    sc = dl.scene_frame()
    tex = [dl.solid_texture((255, 255, 255, 255))]
    for name, world, pixels, tiles in dl.scene_boxes():
        rec = dl.decal_from_box(world, (1, 1))
        _, n = dl.checker(sc, "f32", rec, tex)
        assert n["fade_zero"] + n["fade_partial"] + n["fade_one"] == pixels, name
        P = sc.g[0][..., :3]
        q = np.stack([np.abs(dl_mulcol1(P, rec["invWorld"][0][4 * c:4 * c + 4])) for c in range(3)], -1)
        inside = ((sc.depth & 0xFFFFFF) < 0xFFFFFF) & (q <= 0.5).all(-1)
        assert int(inside.sum()) == pixels, name
        assert int(inside.reshape(12, 8, 16, 8).any((1, 3)).sum()) == tiles, name
        n2 = sc.g[2][..., :3][inside]
        if name in ("floor", "floor_yaw30"):
            assert (n2[:, 1] > 0.99).all(), name                # all up
        if name == "box_face":
            assert (n2[:, 2] < -0.99).all(), name               # all towards -z
    # the normals inside the largest box: 2622 up, 2672 towards -z, 452 along +-x
    assert (int((n2[:, 1] > 0.99).sum()), int((n2[:, 2] < -0.99).sum()), int((np.abs(n2[:, 0]) > 0.99).sum())) == (2622, 2672, 452)


def dl_mulcol1(P, col):
    """mulcol1 in float32, each operation rounded once (numpy has no fma: the products are exact in float64 and rounded once)."""
    x, y, z = (P[..., k].astype(np.float64) for k in range(3))
    c = col.astype(np.float64)
    a = (x * c[0]).astype(np.float32).astype(np.float64)
    a = (y * c[1] + a).astype(np.float32).astype(np.float64)         # one rounding of the exact sum: a 24 x 24-bit product plus a float fits float64 unless the exponents lie far apart
    a = (z * c[2] + a).astype(np.float32)
    return a + col[3]


@pytest.mark.parametrize("name", dl.case_names())
def test_host_body_equals_checker(lib, name):
    k = dl.case_names().index(name)
    _, frame, decals, textures, mix = dl.case(name)
    want, _, passed2 = dl.expected(name)
    got, masks = host_run(frame, mix, decals, textures, misalign=(0, 16, 32)[k % 3], masks=True)
    assert_planes_equal(got, want, name)
    # per tile: the mask holds every decal some pixel of the tile passes step 2 of, and for a tile of finite covered positions no
    # decal whose bounds miss the box of those positions
    H, W = frame.H, frame.W
    P = frame.values(mix)[0][..., :3]
    covered = (frame.depth & 0xFFFFFF) < 0xFFFFFF
    for ty in range(masks.shape[0]):
        for tx in range(masks.shape[1]):
            ys, xs = slice(8 * ty, min(8 * ty + 8, H)), slice(8 * tx, min(8 * tx + 8, W))
            m = int(masks[ty, tx])
            if xs.start >= W:
                assert m == 0
                continue
            need = int(np.bitwise_or.reduce(passed2[ys, xs].reshape(-1)))
            assert need & ~m == 0, "%s tile (%d, %d): the mask %x lacks %x" % (name, tx, ty, m, need & ~m)
            p = P[ys, xs][covered[ys, xs]]
            if len(p) == 0:
                assert m == 0
            elif np.isfinite(p).all():
                lo, hi = p.min(0), p.max(0)
                for d in range(len(decals)):
                    overlap = bool((lo <= decals["boundsMax"][d]).all() and (hi >= decals["boundsMin"][d]).all())
                    assert overlap == bool(m >> d & 1), "%s tile (%d, %d) decal %d" % (name, tx, ty, d)


def test_bounds_touching_the_tile_box_at_one_face_are_in_the_mask(lib):
    sc = dl.scene_frame()
    P = sc.g[0][..., :3]
    covered = (sc.depth & 0xFFFFFF) < 0xFFFFFF
    ty, tx = 9, 10                                       # a tile of floor pixels
    assert covered[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].all()
    p = P[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    rec = dl.decal_from_box(dl.floor_world((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (1, 1))
    tex = [dl.solid_texture((255, 255, 255, 255))]
    for touch, inside in ((True, True), (False, False)):
        rec["boundsMin"][0] = (hi[0], lo[1] - 1, lo[2] - 1) if touch else (np.nextafter(hi[0], np.float32(np.inf)), lo[1] - 1, lo[2] - 1)
        rec["boundsMax"][0] = (hi[0] + 1, hi[1] + 1, hi[2] + 1)
        _, masks = host_run(sc, "f32", rec, tex, masks=True)
        assert bool(masks[ty, tx] & 1) == inside


def test_known_answers(lib):
    sc = dl.scene_frame()
    pristine = sc.planes("f32")
    white = [dl.solid_texture((255, 255, 255, 255))]
    # n = 0 and a decal in the air change nothing
    air = dl.decal_from_box(dl.floor_world((0.0, 30.0, 0.0), (3.0, 1.0, 3.0)), (1, 1), flags=15)
    for decals in (dl.decals_array([]), air):
        assert_planes_equal(host_run(sc, "f32", decals, white), pristine, "unchanged")
    # a 1 x 1 opaque texel, opacity 1, no fade: (tint - x) + x inside the box
    tint = np.array([0.9, 0.5, 0.2], np.float32)
    rec = dl.decal_from_box(dl.floor_world((2.5, 0.0, -7.5), (1.5, 0.25, 1.5)), (1, 1), tint=tint)
    got = host_run(sc, "f32", rec, white)
    inside, outside = dl.inside_box(sc, rec, -1e-4), ~dl.inside_box(sc, rec, 1e-4)
    assert inside.sum() > 400
    x = sc.g[1][..., :3]
    g1 = got[1].view(np.float32)
    assert np.array_equal(g1[inside][:, :3], ((tint[None, None, :] - x) + x)[inside])
    assert np.array_equal(g1[outside], sc.g[1][outside]) and np.array_equal(g1[..., 3], sc.g[1][..., 3])
    assert np.array_equal(got[0], pristine[0]) and np.array_equal(got[2], pristine[2])
    # two overlapping decals: the order shows, and both orders are the checker's
    tex = [dl.solid_texture((255, 255, 255, 200))]
    a = dl.decal_from_box(dl.floor_world((2.5, 0.0, -7.5), (1.5, 0.25, 1.5)), (1, 1), tint=(1.0, 0.0, 0.0))
    b = dl.decal_from_box(dl.floor_world((3.0, 0.0, -7.0), (1.5, 0.25, 1.5)), (1, 1), tint=(0.0, 0.0, 1.0))
    ab, ba = dl.decals_array([a, b]), dl.decals_array([b, a])
    got_ab, got_ba = host_run(sc, "f32", ab, tex), host_run(sc, "f32", ba, tex)
    assert not np.array_equal(got_ab[1], got_ba[1])
    assert_planes_equal(got_ab, dl.checker(sc, "f32", ab, tex)[0], "a then b")
    assert_planes_equal(got_ba, dl.checker(sc, "f32", ba, tex)[0], "b then a")
    # normalW pointing away from the surface: nothing
    down = dl.box_world((2.5, 0.0, -7.5), (1.5, 1.5, 0.25), rot=np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]))
    away = dl.decal_from_box(down, (1, 1), 0.5, 0.0, flags=15)
    assert_planes_equal(host_run(sc, "f32", away, white), pristine, "facing away")


def test_level_rises_with_view_depth_and_addressing_clamps(lib):
    frame, rec, tex = dl.grey_levels_case()
    dl.assert_grey_does_not_fall(frame, rec, host_run(frame, "f32", rec, tex)[1])
    frame, rec, tex = dl.red_blue_case()
    dl.assert_red_blue(host_run(frame, "f32", rec, tex)[1])


@pytest.mark.parametrize("name", ["scene_all_f32", "scene_all_mixed", "scene_all_f16", "130x9_n64_f16", "65x7_n64_mixed", "3x5_n64_mixed"])
def test_row_ranges_stitch_to_the_whole_frame(lib, name):
    _, frame, decals, textures, mix = dl.case(name)
    H = frame.H
    cuts = sorted({0, 1, H // 3, H // 3 + 1, min((2 * H) // 3 | 1, H), H})
    ranges = [(a, b - a) for a, b in zip(cuts, cuts[1:])] + [(H, 0)]
    assert_planes_equal(host_run(frame, mix, decals, textures, ranges=ranges), dl.expected(name)[0], name)
    r0, rn = ranges[1]
    part = host_run(frame, mix, decals, textures, ranges=[(r0, rn)])
    assert_planes_equal(part, dl.checker(frame, mix, decals, textures, r0, rn)[0], name + " rows")
    for p, q in zip(part, frame.planes(mix)):
        assert np.array_equal(p[:r0], q[:r0]) and np.array_equal(p[r0 + rn:], q[r0 + rn:])


# ---- the C ABI's refusals: none needs a context ------------------------------------------------------------------------------------

def test_every_refusal_comes_before_the_context(lib):
    W, H = 16, 8
    buf = np.zeros(W * H * 16 + 64, np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    pcb = lib.PassConstants()
    pcb.View[10], pcb.Proj[5] = 1.0, 2.4
    dec = np.zeros(2, dl.DECAL)
    tex = (lib.Texture * 17)(*[lib.Texture(base, 4, 4, 3) for _ in range(17)])
    good = dict(cb=C.byref(pcb), depth=base, g0=base, g1=base, g2=base, flags=0, decals=dec.ctypes.data, n=2, tex=tex, ntex=1, W=W, H=H, row0=0, rows=H)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.lib.crychic_apply_decals(None, a["cb"], a["depth"], a["g0"], a["g1"], a["g2"], a["flags"], a["decals"], a["n"], a["tex"], a["ntex"],
                                          a["W"], a["H"], a["row0"], a["rows"], None)
        return rc, lib.lib.crychic_last_error().decode()

    assert call() == (-1, "null context")            # everything else is in order: the context is looked at last
    for k in ("cb", "depth", "g0", "g1", "g2", "decals"):
        rc, msg = call(**{k: None})
        assert rc == -1 and "null argument" in msg, k
    assert call(decals=None, n=0) == (-1, "null context")
    for k, off, flags in (("g0", 8, 0), ("g1", 4, 0x2000), ("g2", 8, 0), ("depth", 2, 0), ("decals", dec.ctypes.data + 2 - base, 0)):
        rc, msg = call(**{k: base + off, "flags": flags})
        assert rc == -1 and "aligned" in msg, k
    assert call(g1=base + 8, flags=0x2000) == (-1, "null context")          # a half4 plane needs 8 bytes only
    for kw in (dict(W=0), dict(H=0), dict(row0=1), dict(row0=H + 1, rows=0), dict(rows=H + 1), dict(n=65), dict(ntex=17), dict(flags=0x8000),
               dict(flags=1)):
        rc, msg = call(**kw)
        assert rc == -1 and msg != "null context", kw
    for bad in (lib.Texture(None, 4, 4, 1), lib.Texture(base, 0, 4, 1), lib.Texture(base, 4, 0, 1), lib.Texture(base, 4, 4, 4), lib.Texture(base, 5, 3, 4)):
        rc, msg = call(tex=(lib.Texture * 1)(bad))
        assert rc == -1 and "decal texture 0" in msg
    assert call(tex=(lib.Texture * 1)(lib.Texture(base, 5, 3, 3))) == (-1, "null context")
    rc, msg = call(tex=None)
    assert rc == -1 and "null argument (textures" in msg
    assert call(tex=None, ntex=0) == (-1, "null context")
    rc, msg = call(tex=(lib.Texture * 1)(lib.Texture(base + 2, 4, 4, 1)))
    assert rc == -1 and "decal texture 0 is not 4-byte aligned" in msg
    for field, k, v in (("View", 8, np.inf), ("View", 9, np.nan), ("View", 10, -np.inf), ("View", 11, np.nan), ("Proj", 5, np.nan), ("Proj", 5, np.inf),
                        ("Proj", 5, 0.0)):
        p2 = lib.PassConstants()
        p2.View[10], p2.Proj[5] = 1.0, 2.4
        getattr(p2, field)[k] = v
        rc, msg = call(cb=C.byref(p2))
        assert rc == -1 and field in msg, (field, k)
    rc, msg = call(W=1 << 15, H=(1 << 13) + 1, rows=1)
    assert rc == -4 and "2^28" in msg
    rc, msg = call(tex=(lib.Texture * 1)(lib.Texture(base, 1 << 15, (1 << 13) + 1, 1)))
    assert rc == -4 and "2^28" in msg


# ---- crychic_decal_from_box --------------------------------------------------------------------------------------------------------

def from_box(lib, world, tw=8, th=8, start=1.0, end=1.0):
    d = lib.Decal()
    rc = lib.lib.crychic_decal_from_box((C.c_float * 16)(*[float(x) for x in world]), tw, th, start, end, C.byref(d))
    return rc, d


def test_decal_from_box_known_answers(lib):
    rc, d = from_box(lib, np.eye(4).reshape(16), 8, 4)
    assert rc == 0
    assert list(d.invWorld) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    assert (list(d.tangentW), list(d.bitangentW), list(d.normalW)) == ([1, 0, 0], [0, 1, 0], [0, 0, 1])
    assert d.texelsPerUnit == 8.0 and (d.fadeScale, d.fadeBias) == (0.0, 1.0)
    assert (list(d.tint), d.opacity, d.flags, d.normalTexture, d.texture, d.reserved) == ([1, 1, 1], 1.0, 1, 0xFFFFFFFF, 0, 0)
    pad = 2.0 ** -10 * 1.5
    assert all(-0.5 - 2 * pad < v <= np.float32(-0.5 - pad) for v in d.boundsMin) and all(np.float32(0.5 + pad) <= v < 0.5 + 2 * pad for v in d.boundsMax)
    rc, d = from_box(lib, np.eye(4).reshape(16), 8, 4, 0.5, -0.5)
    assert rc == 0 and (d.fadeScale, d.fadeBias) == (1.0, 0.5)
    # a yaw of 30 degrees, scaled (4, 2, 0.5), centred at (1, 2, 3)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    M = np.eye(4)
    M[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) * np.array([4.0, 2.0, 0.5])[None, :]
    M[:3, 3] = (1, 2, 3)
    M32 = M.astype(np.float32)
    rc, d = from_box(lib, M32.reshape(16), 64, 16)
    assert rc == 0
    inv = np.linalg.inv(M32.astype(np.float64))
    assert np.array_equal(np.array(d.invWorld, np.float32), inv[:3].astype(np.float32).reshape(12)) or \
        np.abs(np.array(d.invWorld, np.float64) - inv[:3].reshape(12)).max() < 2e-8
    assert np.allclose(d.tangentW, [c, 0, -s], atol=1e-7) and np.allclose(d.normalW, [s, 0, c], atol=1e-7) and list(d.bitangentW) == [0, 1, 0]
    assert np.isclose(d.texelsPerUnit, 16.0, rtol=1e-6)            # max(64 / 4, 16 / 2)
    # the bounds hold all eight corners as float32 computes them
    corners = np.array([[x, y, z, 1] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)], np.float32)
    w = np.stack([dl_mulcol1(corners[:, :3], M32[r]) for r in range(3)], -1)
    assert (w >= np.array(d.boundsMin, np.float32)).all() and (w <= np.array(d.boundsMax, np.float32)).all()
    ext = w.max(0) - w.min(0)
    assert (np.array(d.boundsMax) - w.max(0) < 2.0 ** -9 * (ext + np.abs(w).max())).all()


def test_decal_from_box_refusals(lib):
    eye = np.eye(4).reshape(16)
    d = lib.Decal()
    assert lib.lib.crychic_decal_from_box(None, 8, 8, 1.0, 1.0, C.byref(d)) == -1
    assert lib.lib.crychic_decal_from_box((C.c_float * 16)(*eye), 8, 8, 1.0, 1.0, None) == -1
    bad = []
    for k, v in ((0, np.nan), (7, np.inf), (12, 0.5), (15, 2.0)):
        m = eye.copy()
        m[k] = v
        bad.append(m)
    flat = eye.copy()
    flat[10] = 2.0 ** -61                       # an axis shorter than 2^-60
    skew = eye.copy()
    skew[0:12:4] = (0, 1, 0)                    # two equal axes
    for m in bad + [flat, skew]:
        assert from_box(lib, m)[0] == -1
    for tw, th, s, e in ((0, 8, 1, 1), (8, 0, 1, 1), (8, 8, 1.5, 0), (8, 8, 0.5, -1.5), (8, 8, 0.2, 0.4), (8, 8, 0.3, 0.3), (8, 8, np.nan, 0)):
        assert from_box(lib, eye, tw, th, s, e)[0] == -1
