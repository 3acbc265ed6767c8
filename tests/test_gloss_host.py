"""The roughness-prefiltered cube map chain and the glossy reflection lookup on the CPU tier: the product's
sample table against the checker's (tests/gloss_ref), the prefilter body on the host (tests/gloss_host) against the checker byte for
byte, known answers, a float64 numpy restatement of the definition in include/crychic_hip.h that shares no code with either, and the
gloss instantiation of light_pixel on the host against the checker's restated pixel, RGBA8 and radiance bits."""
import ctypes as C

import numpy as np
import pytest

import gloss_lib

KEPT = {3: [26, 16], 4: [29, 22, 16], 5: [30, 26, 20, 16], 9: [32, 30, 28, 26, 23, 20, 18, 16]}
SHAPES = [(16, 5), (8, 4), (12, 3), (20, 3), (64, 7)]       # 16 / 5 ends at 1 x 1; 12 and 20 are ragged: 12-6-3, 20-10-5


@pytest.fixture(scope="module")
def gl():
    return gloss_lib.load()


def _noise_chain(dim, levels, seed=None):
    from crychic_renderer_amd import geometry as g
    cube = np.random.default_rng(1000 + dim if seed is None else seed).integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)
    chain, n = g.cube_mip_chain(cube, levels)
    assert n == levels
    return chain


_REF = {}


def checker_prefilter(gl, dim, levels):
    """The checker's prefilter of the seeded noise chain of a shape, computed once and shared."""
    if (dim, levels) not in _REF:
        src = _noise_chain(dim, levels)
        ref = gl.prefilter(src, dim, levels)
        ref.setflags(write=False)
        _REF[(dim, levels)] = (src, ref)
    return _REF[(dim, levels)]


# ---- the sample table --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", sorted(KEPT))
@pytest.mark.parametrize("dim", [16, 256, 1024])
def test_table_equals_the_checkers_bit_for_bit(built_lib, gl, dim, levels):
    from crychic_renderer_amd import geometry as g
    for k in range(1, levels):
        s, rw = g.cube_prefilter_samples(dim, levels, k)
        ref, n, ref_rw = gl.samples(dim, levels, k)
        assert len(s) == n == KEPT[levels][k - 1], (dim, levels, k)
        assert np.array_equal(s.view(np.uint32), ref[:n].view(np.uint32)), (dim, levels, k)
        assert np.float32(rw).view(np.uint32) == np.float32(ref_rw).view(np.uint32)
        assert (ref[n:] == 0).all()
        assert (s[:, 2] > 0).all()
        assert np.abs(np.linalg.norm(s[:, :3].astype(np.float64), axis=1) - 1.0).max() < 1e-6
        assert (s[:, 3] >= 0).all() and (s[:, 3] <= levels - 1).all()
        assert abs(float(rw) * float(s[:, 2].astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.float32(rw) == np.float32(0.125)          # the last level's weights sum to exactly 8


def test_table_entries_past_the_count_are_zero_and_lod_follows_the_face_size(built_lib):
    lib = built_lib.lib
    s = np.full((32, 4), 7.0, np.float32)
    n, r = C.c_uint32(), C.c_float()
    assert lib.crychic_cube_prefilter_samples(256, 9, 8, s.ctypes.data, C.byref(n), C.byref(r)) == 0
    assert n.value == 16 and (s[16:] == 0).all()
    # four times the texels per solid angle: one level further down, wherever neither lod is clamped
    from crychic_renderer_amd import geometry as g
    a, _ = g.cube_prefilter_samples(256, 9, 4)
    b, _ = g.cube_prefilter_samples(512, 9, 4)
    free = (a[:, 3] > 0) & (b[:, 3] < 8)
    assert free.any() and np.abs(b[free, 3] - a[free, 3] - 1.0).max() < 1e-5
    assert np.array_equal(a[:, :3], b[:, :3])


def test_table_refusals(built_lib):
    lib = built_lib.lib
    s = np.zeros((32, 4), np.float32)
    n, r = C.c_uint32(), C.c_float()
    ok = (s.ctypes.data, C.byref(n), C.byref(r))
    assert lib.crychic_cube_prefilter_samples(16, 5, 1, *ok) == 0
    assert lib.crychic_cube_prefilter_samples(16, 5, 0, *ok) == -1
    assert b"level 0 outside 1 .. 4" in lib.crychic_last_error()
    assert lib.crychic_cube_prefilter_samples(16, 5, 5, *ok) == -1
    assert lib.crychic_cube_prefilter_samples(16, 1, 1, *ok) == -1
    assert lib.crychic_cube_prefilter_samples(0, 5, 1, *ok) == -1
    assert lib.crychic_cube_prefilter_samples(16, 5, 1, None, C.byref(n), C.byref(r)) == -1
    assert lib.crychic_cube_prefilter_samples(16, 5, 1, s.ctypes.data, None, C.byref(r)) == -1
    assert lib.crychic_cube_prefilter_samples(16, 5, 1, s.ctypes.data, C.byref(n), None) == -1
    assert lib.crychic_prefilter_cube_chain(None, None, None, 16, 2, None) == -1       # no context: nothing is computed on the host


# ---- the prefilter body --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,levels", SHAPES)
def test_host_body_equals_the_checker(built_lib, gl, dim, levels):
    src, ref = checker_prefilter(gl, dim, levels)
    got, n = gl.host_prefilter(src, dim, levels)
    assert n == ref.size and np.array_equal(got[:n], ref)
    assert (got[n:] == 0xA5).all()
    assert np.array_equal(ref[:6 * dim * dim * 4], src[:6 * dim * dim * 4])        # level 0 is copied


def test_host_body_of_a_one_level_chain_copies_it(built_lib, gl):
    src = _noise_chain(8, 1, seed=3)
    got, n = gl.host_prefilter(src, 8, 1)
    assert np.array_equal(got[:n], src) and (got[n:] == 0xA5).all()
    assert np.array_equal(gl.prefilter(src, 8, 1), src)


def test_a_single_colour_stays_that_colour(built_lib, gl):
    colour = np.array([200, 3, 97, 255], np.uint8)
    dim, levels = 16, 5
    src = np.tile(colour, gloss_lib.chain_bytes(dim, levels) // 4)
    assert np.array_equal(gl.prefilter(src, dim, levels), src)
    assert np.array_equal(gl.host_prefilter(src, dim, levels)[0][:src.size], src)


def _texel_directions(d):
    """(6, d, d, 3) float64: the direction of each texel centre, by the face table of include/crychic_hip.h."""
    c = (2.0 * np.arange(d) + 1.0) / d - 1.0
    t, s = np.meshgrid(c, c, indexing="ij")        # [y, x]
    one = np.ones_like(s)
    return np.stack([np.stack(v, -1) for v in ((one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one))])


def _edge_profile(level, d):
    """The middle row of faces +X, +Y and -X of a level, as (angle from +X towards +Y in the xy plane, red channel), sorted by angle."""
    dirs = _texel_directions(d)
    ang, val = [], []
    for f in (0, 2, 1):
        # +X and -X: the row y = d // 2 runs along z, the column x = d // 2 is the one in the xy plane (z ~ 0); +Y likewise its row
        for i in range(d):
            x, y = (d // 2, i) if f in (0, 1) else (i, d // 2)
            v = dirs[f, y, x]
            a = np.arctan2(v[1] + 0.0, v[0])        # -0 + 0 = +0: the centre of -X is at pi, not -pi
            if a >= -1e-12:
                ang.append(a); val.append(int(level[f, y, x, 0]))
    o = np.argsort(ang, kind="stable")
    return np.array(ang)[o], np.array(val, np.float64)[o]


def _crossing(ang, val, thr):
    """The angle at which the non-increasing profile first falls to `thr`, by linear interpolation between texel centres."""
    for i in range(1, len(val)):
        if val[i] <= thr < val[i - 1]:
            return ang[i - 1] + (ang[i] - ang[i - 1]) * (val[i - 1] - thr) / (val[i - 1] - val[i])
    return ang[0] if val[0] <= thr else ang[-1]


def test_one_white_face_blurs_monotonically_and_ever_wider(built_lib, gl):
    """+X white, the others black; the walk goes from the centre of +X over the edge to +Y and on to the centre of -X in the xy plane
    (where the tangent frame never switches its up vector).  Across the edge -- the halves of +X and +Y that border it, 22.5 to 67.5
    degrees -- the red channel never rises, at any level; and the 10-90 % width of the fall, in level-0 texels, does not shrink from
    one level to the next.  The step's height is known (white to black), so the width is the stretch of the walk on which the
    profile lies between 90 % and 10 % of 255; a level that is below 90 % already at the centre of the white face starts at the
    centre, one that never falls to 10 % ends with the walk.
    Monotony is asserted across the edge and not over the whole walk: at the centre of the white face the exact profile is flat by
    symmetry, and there the 32 fixed samples of the definition decide the sign of a step (one sample is worth up to 12 LSB at level
    3: the checker's level 3 of this cube map reads 163, 171, 153, ... from the centre outwards).  The width is read off the texel
    centres by linear interpolation, so the last level keeps 4 x 4 texels a face: a walk over three texels 90 degrees apart would
    measure their spacing and not the blur."""
    from crychic_renderer_amd import geometry as g
    dim, levels = 64, 5
    cube = np.zeros((6, dim, dim, 4), np.uint8)
    cube[0] = 255
    src, _ = g.cube_mip_chain(cube, levels)
    out = gl.prefilter(src, dim, levels)
    widths = []
    for k in range(levels):
        d = max(dim >> k, 1)
        ang, val = _edge_profile(gloss_lib.level_view(out, dim, k), d)
        print("level", k, val.astype(int).tolist())
        edge = (ang >= np.pi / 8) & (ang <= 3 * np.pi / 8)
        assert edge.sum() >= 2 and (np.diff(val[edge]) <= 0).all(), (k, val[edge])
        a90, a10 = _crossing(ang, val, 0.9 * 255), _crossing(ang, val, 0.1 * 255)
        widths.append((a10 - a90) / (np.pi / 2) * dim)
    print("10-90 % widths in level-0 texels:", widths)
    assert all(b >= a for a, b in zip(widths, widths[1:])), widths


# ---- a float64 restatement of the definition, sharing nothing with the checker ---------------------------------------------------

def _np_table(dim, levels, k):
    a2 = (k / (levels - 1.0)) ** 2
    i = np.arange(32)
    xi1 = (i + 0.5) / 32
    xi2 = np.array([int(format(v, "05b")[::-1], 2) / 32.0 for v in i])
    cos2 = (1 - xi1) / (1 + (a2 - 1) * xi1)
    w = 2 * cos2 - 1
    keep = w > 0
    cs = 2 * np.sqrt(cos2) * np.sqrt(1 - cos2)
    D = a2 / (np.pi * ((a2 - 1) * cos2 + 1) ** 2)
    lod = np.clip(0.5 * np.log2((1 / (32 * D / 4)) / (4 * np.pi / (6.0 * dim * dim))) + 1, 0, levels - 1)
    t = np.stack([cs * np.cos(2 * np.pi * xi2), cs * np.sin(2 * np.pi * xi2), w, lod], -1)[keep]
    return t.astype(np.float32).astype(np.float64), float(np.float32(1.0 / w[keep].sum()))       # stored as float


def _np_cube_linear(level, r):
    """Bilinear lookup inside the face of r (major axis, ties x >= y >= z), clamp to edge: level (6, d, d, 4) float64, r (n, 3)."""
    d = level.shape[1]
    ax, ay, az = np.abs(r[:, 0]), np.abs(r[:, 1]), np.abs(r[:, 2])
    isx = (ax >= ay) & (ax >= az)
    isy = ~isx & (ay >= az)
    px, py, pz = r[:, 0] >= 0, r[:, 1] >= 0, r[:, 2] >= 0
    ma = np.where(isx, ax, np.where(isy, ay, az))
    sc = np.where(isx, np.where(px, -r[:, 2], r[:, 2]), np.where(isy, r[:, 0], np.where(pz, r[:, 0], -r[:, 0])))
    tc = np.where(isx, -r[:, 1], np.where(isy, np.where(py, r[:, 2], -r[:, 2]), -r[:, 1]))
    face = np.where(isx, np.where(px, 0, 1), np.where(isy, np.where(py, 2, 3), np.where(pz, 4, 5)))
    tx, ty = 0.5 * (sc / ma + 1) * d - 0.5, 0.5 * (tc / ma + 1) * d - 0.5
    x0, y0 = np.floor(tx), np.floor(ty)
    fx, fy = (tx - x0)[:, None], (ty - y0)[:, None]
    cl = lambda v: np.clip(v, 0, d - 1).astype(np.int64)
    t00, t10 = level[face, cl(y0), cl(x0)], level[face, cl(y0), cl(x0 + 1)]
    t01, t11 = level[face, cl(y0 + 1), cl(x0)], level[face, cl(y0 + 1), cl(x0 + 1)]
    top, bot = t00 + fx * (t10 - t00), t01 + fx * (t11 - t01)
    return top + fy * (bot - top)


# Steps 1 to 3 of the definition fix the binary32 operations that lead to a sample's direction, and which face a direction on a
# face edge belongs to is decided by its last bit (diagonal texels and the samples at phi = pi / 2 meet the x = y edges exactly;
# nothing is filtered across faces, so the two sides differ by many LSB at the small levels).  The frame and the direction are
# therefore restated in binary32 -- numpy's float32 operations, a mad as the float64 sum rounded once more -- and everything a
# rounding cannot flip (the table, the lookups, the sum) in float64.
def _mad(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _normalize32(v):
    d2 = _mad(v[:, 2], v[:, 2], _mad(v[:, 1], v[:, 1], v[:, 0] * v[:, 0]))
    inv = np.float32(1) / np.sqrt(np.clip(d2, np.float32(2.0 ** -100), np.float32(2.0 ** 100)))
    return v * inv[:, None]


def _cross32(a, b):
    return np.stack([_mad(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), _mad(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])),
                     _mad(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], -1)


def _np_prefilter(chain, dim, levels):
    lv = [gloss_lib.level_view(chain, dim, k).astype(np.float64) / 255.0 for k in range(levels)]
    out = [gloss_lib.level_view(chain, dim, 0).astype(np.float64)]
    for k in range(1, levels):
        d = max(dim >> k, 1)
        tab, rw = _np_table(dim, levels, k)
        c = (2 * np.arange(d) + 1).astype(np.float32) * (np.float32(1) / np.float32(d)) - np.float32(1)
        t, s = np.meshgrid(c, c, indexing="ij")
        one = np.ones_like(s)
        N = np.stack([np.stack(v, -1) for v in ((one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one))])
        N = _normalize32(N.reshape(-1, 3))
        up = np.where((np.abs(N[:, 2]) < np.float32(0.999))[:, None], np.float32([0, 0, 1]), np.float32([1, 0, 0]))
        T = _normalize32(_cross32(up, N))
        B = _cross32(N, T)
        acc = np.zeros((N.shape[0], 4))
        for lx, ly, lz, lod in tab:
            e = np.float32([lx, ly, lz])
            L = np.stack([_mad(e[2], N[:, j], _mad(e[1], B[:, j], e[0] * T[:, j])) for j in range(3)], -1).astype(np.float64)
            l0 = int(lod)
            c = _np_cube_linear(lv[l0], L)
            if lod > l0 and l0 + 1 < levels:
                c = c + (lod - l0) * (_np_cube_linear(lv[l0 + 1], L) - c)
            acc += lz * c
        out.append(np.clip(acc * rw, 0, 1) * 255.0)
    return out


def test_numpy_restatement_within_one_lsb(built_lib, gl):
    """The fp32 error of a 32-term weighted mean is about 1e-5, far below 1 / 255: only a rounding boundary separates the checker's
    bytes from round(the float64 value)."""
    from crychic_renderer_amd import geometry as g
    dim, levels = 16, 5
    dirs = _texel_directions(dim)
    dirs = dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)
    rng = np.random.default_rng(77)
    cube = np.zeros((6, dim, dim, 4), np.uint8)
    for c in range(4):           # smooth: a low-frequency function of the direction, continuous across the face edges
        a, ph = rng.normal(size=3) * 1.5, rng.uniform(0, 6.28)
        cube[..., c] = np.round(127.5 + 110.0 * np.sin(dirs @ a + ph)).astype(np.uint8)
    src, _ = g.cube_mip_chain(cube, levels)
    ref = gl.prefilter(src, dim, levels)
    exact = _np_prefilter(src, dim, levels)
    worst = 0.0
    for k in range(levels):
        d = max(dim >> k, 1)
        err = np.abs(gloss_lib.level_view(ref, dim, k).astype(np.float64) - exact[k].reshape(6, d, d, 4))
        worst = max(worst, err.max())
        # a byte is round(value): it is within half an LSB of the float64 value, plus the fp32 error of the sum
        assert err.max() <= 0.5 + 255 * 1e-4, (k, err.max())
        assert np.abs(gloss_lib.level_view(ref, dim, k).astype(np.int64) - np.floor(exact[k].reshape(6, d, d, 4) + 0.5).astype(np.int64)).max() <= 1
    print("largest |checker byte - float64 value| in LSB:", worst)


# ---- the gloss lookup of the lighting pass (CRYCHIC_LIGHT_CUBE_GLOSS) -------------------------------------------------------------

GLOSS = gloss_lib.GLOSS
SIZES = [(64, 48), (70, 38)]          # 70 x 38: a ragged last workgroup column and row on the device


def levels_flag(n):
    return (n & 15) << 16


def edge_roughness(levels):
    """0, 1, every k / (n - 1) and one ulp either side of it, values below 0 and above 1, -0 and NaN."""
    v = [0.0, 1.0, -0.0, -0.5, -1e30, 1.5, 3e38, np.nan, -np.inf, np.inf, 0.37, 0.9999]
    for k in range(levels):
        x = np.float32(k / (levels - 1.0))
        v += [x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2))]
    return np.array(v, np.float32)


def with_edge_roughness(p, levels):
    """The planes with the roughness edge values cycling through G1.w (every value lands on covered pixels of any frame row)."""
    g1 = p["g1"].copy()
    v = edge_roughness(levels)
    H, W = g1.shape[:2]
    g1[..., 3] = v[(np.arange(H)[:, None] * 7 + np.arange(W)[None, :]) % len(v)]
    return dict(p, g1=g1)


_CHAINS = {}


def gloss_chain(gl, p, levels):
    """(the prefiltered chain the frames of `levels` levels bind, its face size): the scene's 32-texel cube map for chains of 2 and 5
    levels, seeded noise of 256 for 9."""
    from crychic_renderer_amd import geometry as g
    if levels not in _CHAINS:
        if levels == 9:
            _CHAINS[levels] = (checker_prefilter(gl, 256, 9)[1], 256)
        else:
            box, n = g.cube_mip_chain(p["cube"], levels)
            assert n == levels
            chain = gl.prefilter(box, 32, levels)
            chain.setflags(write=False)
            _CHAINS[levels] = (chain, 32)
    return _CHAINS[levels]


def same_frame(a, b):
    from fuzz_util import same_floats
    return np.array_equal(a[0], b[0]) and same_floats(a[1], b[1])


@pytest.mark.parametrize("levels", [2, 5, 9])
@pytest.mark.parametrize("W,H", SIZES)
def test_gloss_body_matches_checker_without_local_lights(built_lib, gl, W, H, levels):
    """The host body == the checker, RGBA8 and radiance bits (a NaN roughness makes `shininess` NaN: any NaN equals any NaN), with
    the roughness edge values, both PCF radii, Q fixes off and on, sky on and off."""
    from local_lights_util import FIX_ALL, _cpu
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, levels)
    q = dict(with_edge_roughness(p, levels), cube=chain)
    for fixes, ndl, radius, sky in ((0, 1, 0.0, 1), (FIX_ALL, 3, 2.5 / 256, 0)):
        flags = fixes | sky | GLOSS | levels_flag(levels)
        got = gl.host_light(c.pass_cb, q, None, ndl, radius, flags, cube_dim=dim)
        ref = gl.checker_light(pcb, q, None, ndl, radius, flags, cube_dim=dim)
        assert same_frame(got, ref), (fixes, levels)
    lit = (p["depth"] & 0xFFFFFF) < 0xFFFFFF
    assert lit.any() and (~lit).any()


@pytest.mark.parametrize("levels", [2, 5, 9])
def test_gloss_body_matches_checker_with_local_lights_and_shadows(built_lib, gl, levels):
    """Points, spots, 3 shadowed spots and 2 shadowed points; then the same without any shadow; both sizes, both radii."""
    from local_lights_util import FIX_ALL
    from test_point_shadows import _frame_setup
    for (W, H), radius, fixes in zip(SIZES, (0.0, 0.01), (0, FIX_ALL)):
        p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, 2, 48, 3, seed=levels)
        chain, dim = gloss_chain(gl, p, levels)
        q = dict(with_edge_roughness(p, levels), cube=chain)
        flags = fixes | 1 | GLOSS | levels_flag(levels)
        for args in (dict(points=points, spots=spots, maps=maps, cubes=cubes, projs=projs), dict(points=points, spots=spots), dict(points=points)):
            got = gl.host_light(cb, q, None, 3, radius, flags, cube_dim=dim, **args)
            ref = gl.checker_light(pcb, q, None, 3, radius, flags, cube_dim=dim, **args)
            assert same_frame(got, ref), (W, H, levels, sorted(args))


def test_gloss_body_matches_checker_on_a_half_float_mix(built_lib, gl):
    """G0 float4 with G1 and G2 half4: the body on the packed planes == the checker on the widened planes (the roughness the lookup
    takes is the decoded value)."""
    import gbuffer_f16_lib as gf
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, 5)
    packed = gf.pack_planes(dict(with_edge_roughness(p, 5), cube=chain), gf.MIXED)
    wide = gf.widen_planes(packed)
    flags = 1 | GLOSS | levels_flag(5)
    got = gl.host_light(c.pass_cb, packed, None, 3, 0.0, flags, cube_dim=dim, formats=True)
    ref = gl.checker_light(pcb, wide, None, 3, 0.0, flags, cube_dim=dim)
    assert same_frame(got, ref)


def test_gloss_sky_is_level_0_and_roughness_picks_the_level(built_lib, gl, oracle):
    """Under the flag the sky pixels are those of the level-0 call; and a frame whose roughness is k / (n - 1) everywhere reads level k
    alone: it equals the level-0 frame (the frozen oracle's) over level k bound as a cube map of its own."""
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, pcb = _cpu(W, H)
    levels = 5
    chain, dim = gloss_chain(gl, p, levels)
    sky = (p["depth"] & 0xFFFFFF) == 0xFFFFFF
    base = oracle.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], None, p["shadow"], gloss_lib.level_view(chain, dim, 0).copy(), 3, 0.0, sky=True)
    ref = gl.checker_light(pcb, dict(p, cube=chain), None, 3, 0.0, 1 | GLOSS | levels_flag(levels), cube_dim=dim)
    assert sky.any() and np.array_equal(ref[0][sky], base[sky])
    for k in (0, 2, 4):
        g1 = p["g1"].copy()
        g1[..., 3] = np.float32(k / 4.0)
        one = oracle.deferred_light(pcb, p["g0"], g1, p["g2"], p["depth"], None, p["shadow"], gloss_lib.level_view(chain, dim, k).copy(), 3, 0.0, sky=True)
        got = gl.checker_light(pcb, dict(p, g1=g1, cube=chain), None, 3, 0.0, 1 | GLOSS | levels_flag(levels), cube_dim=dim)
        assert np.array_equal(got[0][~sky], one[~sky]), k


def test_gloss_over_a_chain_of_equal_levels_is_the_level_0_frame(built_lib, gl, oracle):
    """Every level of the chain holds the same image -- six faces of one colour each, the only image that levels of different sizes
    can share: whatever level the roughness selects, the lookup returns what level 0 does, so the gloss frame (checker and host
    body) is the level-0 frame of the frozen oracle, bit for bit.  The lookup is the only change."""
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    levels, dim = 5, 32
    colours = np.array([[250, 10, 20, 255], [10, 240, 30, 255], [15, 25, 230, 255], [200, 200, 10, 255], [10, 190, 210, 255], [128, 64, 32, 255]], np.uint8)
    chain = np.concatenate([np.repeat(colours[:, None, :], max(dim >> k, 1) ** 2, axis=1).reshape(-1) for k in range(levels)])
    q = with_edge_roughness(p, levels)
    flags = 1 | GLOSS | levels_flag(levels)
    base, rbase = oracle.deferred_light(pcb, q["g0"], q["g1"], q["g2"], q["depth"], None, q["shadow"], gloss_lib.level_view(chain, dim, 0).copy(), 3,
                                        0.0, sky=True, want_radiance=True)
    for fn, cb in ((gl.checker_light, pcb), (gl.host_light, c.pass_cb)):
        got = fn(cb, dict(q, cube=chain), None, 3, 0.0, flags, cube_dim=dim)
        assert same_frame(got, (base, rbase))


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_gloss_fuzz_planes_through_checker_and_body(built_lib, gl, seed):
    """fuzz_util's planes (NaN, inf, zero-length vectors, NaN roughness) with the flag set: the host body == the checker."""
    import fuzz_util
    import oracle_lib
    from crychic_renderer_amd import geometry as g
    W, H, planes, c, knobs = fuzz_util.random_case(seed, built_lib)
    chain, levels = g.cube_mip_chain(planes["cube"])
    dim = planes["cube"].shape[1]
    if levels < 2:
        pytest.fail("the fuzz cube map has no chain")
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    q = dict(planes, cube=chain)
    flags = knobs["sky"] | GLOSS | levels_flag(levels)
    got = gl.host_light(c.pass_cb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)
    ref = gl.checker_light(pcb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)
    assert same_frame(got, ref)
