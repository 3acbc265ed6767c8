"""CPU tier of the SH9 irradiance (include/crychic_hip.h "SH9 irradiance"): the bodies of cube_sh.hip and of the
AmbientSH lighting kernels, built for the host (tests/env_sh_host), against the checker (tests/env_sh_ref) bit for bit; the
properties of the definition; a float64 restatement; the tie to the frozen oracle; the binding's refusals."""
import numpy as np
import pytest

import env_sh_lib
from env_sh_lib import AMBIENT_SH, TAIL_BYTES, tail_offset, with_tail

DIMS = [1, 2, 5, 16, 64]


@pytest.fixture(scope="module")
def es():
    return env_sh_lib.load()


def noise_level(d, seed=None):
    return np.random.default_rng(1000 + d if seed is None else seed).integers(0, 256, (6, d, d, 4), dtype=np.uint8)


def smooth_level(d):
    """A sky-like gradient with a warm patch: smooth in the direction, different per channel."""
    n = _directions64(d)
    up, side = n[..., 1], n[..., 0]
    rgb = np.stack([0.35 + 0.3 * up + 0.25 * np.maximum(side, 0) ** 4, 0.4 + 0.35 * up, 0.55 + 0.4 * up - 0.1 * side], -1)
    out = np.full((6, d, d, 4), 255, np.uint8)
    out[..., :3] = np.floor(np.clip(rgb, 0, 1) * 255 + 0.5).astype(np.uint8)
    return out


def _directions64(d):
    """(6, d, d, 3) float64 unnormalised texel-centre directions divided by their length; written without the checker's helpers."""
    c = (2.0 * np.arange(d) + 1.0) / d - 1.0
    s, t = np.meshgrid(c, c, indexing="xy")          # s along x (columns), t along y (rows)
    one = np.ones_like(s)
    faces = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]
    v = np.stack([np.stack(f, -1) for f in faces])
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def block_of(tail):
    return tail[:144].view(np.float32).reshape(9, 4)


# ---- the projection ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", DIMS)
def test_host_body_equals_the_checker_bit_for_bit(es, d):
    """Noise cubes and cubes of 0 and 255: the 28 sums and the 36 floats; the tail's pre-fill (0xFF, then 0x00) does not matter, the
    bytes past the accumulators are left alone, and every fourth component is +0."""
    for level in (noise_level(d), noise_level(d, 7), np.zeros((6, d, d, 4), np.uint8), np.full((6, d, d, 4), 255, np.uint8)):
        ref = es.project(level)
        assert np.array_equal(es.sums(level), es.sums(level, host=True))
        for fill in (0xFF, 0x00):
            tail = es.host_project(level, fill=fill)
            assert np.array_equal(bits(block_of(tail)), bits(ref))
            assert np.array_equal(tail[144:368].view(np.int64), es.sums(level)) and (tail[368:] == fill).all()
        assert not bits(ref[:, 3]).any()
    zero = es.project(np.zeros((6, d, d, 4), np.uint8))
    assert not bits(zero).any()


@pytest.mark.parametrize("d", DIMS)
def test_the_sums_do_not_depend_on_how_the_texels_are_grouped(es, d):
    """Two subsets added give the whole (on the body's accumulate function), and so does any number of simulated workgroups."""
    level = noise_level(d)
    n = 6 * d * d
    whole = es.sums(level, host=True)
    for cut in sorted({0, 1, n // 3, n // 2 + 1, n - 1, n} & set(range(n + 1))):
        assert np.array_equal(es.sums(level, 0, cut, host=True) + es.sums(level, cut, n, host=True), whole)
    ref = es.project(level)
    for blocks in (1, 2, 3, 7, 96):
        assert np.array_equal(bits(block_of(es.host_project(level, blocks=blocks))), bits(ref)), blocks


@pytest.mark.parametrize("d", DIMS)
def test_a_cube_of_one_colour_has_that_ambient_colour(es, d):
    """C0 == (float)(c / 255.0) exactly; for d a power of two every texel has a mirror texel whose term is the exact negation, so
    C1..C5 and C7 are exactly 0 (the checker confirms it; at d = 5 (2x + 1) / 5 - 1 is not symmetric in binary32 and they are not)."""
    for c in ((255, 255, 255), (0, 0, 0), (77, 200, 1), (128, 3, 254)):
        level = np.zeros((6, d, d, 4), np.uint8)
        level[..., :3] = c
        level[..., 3] = 99                                     # alpha is ignored
        co = es.project(level)
        assert np.array_equal(co[0, :3], (np.array(c, np.float64) / 255.0).astype(np.float32))
        if d & (d - 1) == 0:
            assert not co[[1, 2, 3, 4, 5, 7]].any()
        assert np.array_equal(bits(block_of(es.host_project(level))), bits(co))


def test_a_white_top_face_lights_from_above(es):
    for d in (5, 16, 64):
        level = np.zeros((6, d, d, 4), np.uint8)
        level[2] = 255
        co = es.project(level)
        up, side, down = (es.irradiance(co, n)[0] for n in ((0, 1, 0), (1, 0, 0), (0, -1, 0)))
        assert up > side > down >= 0.0


def _np_project(level):
    """The definition in float64 without quantisation: texel-centre weights 1 / r^3, the nine monomials, K."""
    d = level.shape[1]
    c = (2.0 * np.arange(d) + 1.0) / d - 1.0
    s, t = np.meshgrid(c, c, indexing="xy")
    r2 = 1.0 + s * s + t * t
    w = np.broadcast_to(r2 ** -1.5, (6, d, d))
    n = _directions64(d)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    b = np.stack([np.ones_like(x), y, z, x, x * y, y * z, 3.0 * z * z - 1.0, x * z, x * x - y * y])      # (9, 6, d, d)
    texel = level[..., :3].astype(np.float64)
    num = np.einsum("mfyx,fyx,fyxc->mc", b, w, texel)
    return num * env_sh_lib.K[:, None] / (w.sum() * 255.0)


def test_float64_restatement_within_the_derived_bound(es):
    """|C_m(checker) - C_m(float64)| <= 6e-6 K_m: each term is rounded by at most 1 unit (half a unit of quantisation, the binary32
    product and weight) against a mean weight of about 0.52 * 2^20, in numerator and denominator.  Largest difference seen here,
    in units of K_m: 1.4e-8 (smooth, d = 64), 2.1e-8 (noise, d = 16), 5.2e-8 (noise, d = 5), 1.7e-7 (smooth, d = 2) -- at these
    sizes mostly the rounding of C_m to binary32."""
    worst = 0.0
    for level in (smooth_level(64), noise_level(16), noise_level(5), smooth_level(2)):
        got, ref = es.project(level)[:, :3].astype(np.float64), _np_project(level)
        rel = np.abs(got - ref).max(axis=1) / env_sh_lib.K
        worst = max(worst, rel.max())
        print("d = %d: largest |dC_m| / K_m = %.3g" % (level.shape[1], rel.max()))
        assert (rel <= 6e-6).all()
    assert worst > 0.0


# ---- the lighting pass -------------------------------------------------------------------------------------------------------------

from test_gloss_host import GLOSS, SIZES, gloss_chain, levels_flag, same_frame, with_edge_roughness  # noqa: E402

EDGE_NORMALS = np.array([[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [-np.inf, 1, 0], [0, 3, 4], [1e-3, 2e-3, -1e-3], [1e20, 0, 0], [0, -1, 0],
                         [1e-30, 0, 0], [-0.0, 0, -0.0], [np.inf, np.inf, 0], [0.6, 0, 0.8]], np.float32)


def with_edge_normals(p):
    """Zero-length, NaN, +-inf, non-unit and tiny normals on every third pixel, the scene's own on the others."""
    g2 = p["g2"].copy()
    H, W = g2.shape[:2]
    k = np.arange(H)[:, None] * 5 + np.arange(W)[None, :]
    sel = k % 3 == 0
    g2[..., :3][sel] = EDGE_NORMALS[(k // 3) % len(EDGE_NORMALS)][sel]
    return dict(p, g2=g2)


def scene_block(es, p):
    """The coefficient block of the scene's own cube map (level 0 of p["cube"])."""
    return es.project(p["cube"])


def edge_blocks(es, p):
    """The scene's block, and blocks that make e negative, NaN, +inf and -inf on some or all normals."""
    base = scene_block(es, p)
    neg = base.copy(); neg[0, :3] = (-0.5, 0.1, -2.0); neg[1, :3] = (0.9, -0.9, 0.3)
    nan = base.copy(); nan[4, 0] = np.nan; nan[0, 1] = np.nan
    inf = base.copy(); inf[2, 0] = np.inf; inf[0, 1] = -np.inf; inf[8, 2] = np.inf
    big = (base * np.float32(1e38)).astype(np.float32)
    return [base, neg, nan, inf, big]


def cube_for(es, p, levels):
    """(the cube map the flag's frames of `levels` levels bind, its face size): the scene's own for no chain, test_gloss_host's
    prefiltered chains for 2 and 5."""
    if levels <= 1:
        return np.ascontiguousarray(p["cube"]).reshape(-1), p["cube"].shape[1]
    return gloss_chain(env_sh_lib.gloss_lib.load(), p, levels)


def sh_flags(levels):
    return AMBIENT_SH | (GLOSS | levels_flag(levels) if levels > 1 else 0)


@pytest.mark.parametrize("levels", [0, 2, 5])
@pytest.mark.parametrize("W,H", SIZES)
def test_sh_body_matches_checker_without_local_lights(built_lib, es, W, H, levels):
    """The host body == the checker, RGBA8 and radiance bits: no chain and gloss chains, the edge normals and roughness values, every
    edge coefficient block, both PCF radii, Q fixes off and on, sky on and off."""
    from local_lights_util import FIX_ALL, _cpu
    _, p, c, pcb = _cpu(W, H)
    cube, dim = cube_for(es, p, levels)
    q = with_edge_normals(with_edge_roughness(p, max(levels, 2)))
    for k, block in enumerate(edge_blocks(es, p)):
        fixes, ndl, radius, sky = ((0, 1, 0.0, 1), (FIX_ALL, 3, 2.5 / 256, 0))[k & 1]
        flags = fixes | sky | sh_flags(levels)
        qq = dict(q, cube=with_tail(cube, dim, levels, block))
        got = es.host_light(c.pass_cb, qq, None, ndl, radius, flags, cube_dim=dim)
        ref = es.checker_light(pcb, qq, None, ndl, radius, flags, cube_dim=dim)
        assert same_frame(got, ref), (levels, k)
    lit = (p["depth"] & 0xFFFFFF) < 0xFFFFFF
    assert lit.any() and (~lit).any()


@pytest.mark.parametrize("levels", [0, 5])
def test_sh_body_matches_checker_with_local_lights_and_shadows(built_lib, es, levels):
    """Points, spots, 3 shadowed spots and 2 shadowed points; then the same without any shadow; both sizes, both radii."""
    from local_lights_util import FIX_ALL
    from test_point_shadows import _frame_setup
    for (W, H), radius, fixes in zip(SIZES, (0.0, 0.01), (0, FIX_ALL)):
        p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, 2, 48, 3, seed=3 + levels)
        cube, dim = cube_for(es, p, levels)
        q = dict(with_edge_normals(with_edge_roughness(p, max(levels, 2))), cube=with_tail(cube, dim, levels, scene_block(es, p)))
        flags = fixes | 1 | sh_flags(levels)
        for args in (dict(points=points, spots=spots, maps=maps, cubes=cubes, projs=projs), dict(points=points, spots=spots), dict(points=points)):
            got = es.host_light(cb, q, None, 3, radius, flags, cube_dim=dim, **args)
            ref = es.checker_light(pcb, q, None, 3, radius, flags, cube_dim=dim, **args)
            assert same_frame(got, ref), (W, H, levels, sorted(args))


def test_sh_body_matches_checker_on_a_half_float_mix_and_with_an_ambient_map(built_lib, es):
    """G0 float4 with G1 and G2 half4: the body on the packed planes == the checker on the widened planes; then float planes with a
    half-res ambient map (ambientAccess != 1)."""
    import gbuffer_f16_lib as gf
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    for levels in (0, 5):
        cube, dim = cube_for(es, p, levels)
        q = dict(with_edge_normals(with_edge_roughness(p, 5)), cube=with_tail(cube, dim, levels, scene_block(es, p)))
        packed = gf.pack_planes(q, gf.MIXED)
        wide = gf.widen_planes(packed)
        flags = 1 | sh_flags(levels)
        got = es.host_light(c.pass_cb, packed, None, 3, 0.0, flags, cube_dim=dim, formats=True)
        assert same_frame(got, es.checker_light(pcb, wide, None, 3, 0.0, flags, cube_dim=dim))
        ao = np.random.default_rng(levels).integers(0, 65536, (H // 2, W // 2), dtype=np.uint16)
        got = es.host_light(c.pass_cb, q, ao, 3, 0.0, flags, cube_dim=dim)
        assert same_frame(got, es.checker_light(pcb, q, ao, 3, 0.0, flags, cube_dim=dim))


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_sh_fuzz_planes_through_checker_and_body(built_lib, es, seed):
    """fuzz_util's planes (NaN, inf, zero-length vectors) with the flag set, no chain and the box chain taken as a gloss chain."""
    import fuzz_util
    import oracle_lib
    from crychic_renderer_amd import geometry as g
    W, H, planes, c, knobs = fuzz_util.random_case(seed, built_lib)
    chain, levels = g.cube_mip_chain(planes["cube"])
    dim = planes["cube"].shape[1]
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    block = es.project(planes["cube"])
    for n, cube in ((0, np.ascontiguousarray(planes["cube"]).reshape(-1)), (levels, chain)):
        if n == 1:
            continue
        q = dict(planes, cube=with_tail(cube, dim, n, block))
        flags = knobs["sky"] | sh_flags(n)
        got = es.host_light(c.pass_cb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)
        ref = es.checker_light(pcb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)
        assert same_frame(got, ref), n


def test_a_constant_block_of_the_ambient_light_is_the_frozen_oracles_frame(built_lib, es, oracle):
    """C0 = AmbientLight.rgb and C1..C8 = 0: e = C0 on every pixel with a finite normal (fma(0, b, e) = e), so the flag's frame --
    checker and host body -- is the frozen oracle's frame, bit for bit, with no chain.  The new path meets the old one."""
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    q = with_edge_roughness(p, 5)
    block = np.zeros((9, 4), np.float32)
    block[0, :3] = np.array(c.pass_cb.AmbientLight[:3], np.float32)
    assert block[0, :3].any()
    cube, dim = cube_for(es, p, 0)
    base, rbase = oracle.deferred_light(pcb, q["g0"], q["g1"], q["g2"], q["depth"], None, q["shadow"], p["cube"], 3, 0.0, sky=True, want_radiance=True)
    qq = dict(q, cube=with_tail(cube, dim, 0, block))
    for fn, cb in ((es.checker_light, pcb), (es.host_light, c.pass_cb)):
        assert same_frame(fn(cb, qq, None, 3, 0.0, 1 | AMBIENT_SH, cube_dim=dim), (base, rbase))
    # ... and the scene's own block gives another frame: the flag bites
    other = es.checker_light(pcb, dict(q, cube=with_tail(cube, dim, 0, scene_block(es, p))), None, 3, 0.0, 1 | AMBIENT_SH, cube_dim=dim)
    assert (other[0] != base).any()


def test_refusals_of_the_binding_and_the_size_functions(built_lib, es):
    """The flag with a derivative chain, a null cube map and a misaligned tail are refused by light_bind.hpp's check; the size
    functions of the library, the harness and the checker agree; a buffer one byte short of the tail is short."""
    lib = built_lib.lib
    a = 0x10000
    assert es.check(AMBIENT_SH, a, 32) == 0 and es.check(0, 0, 32) == 0
    assert es.check(AMBIENT_SH | GLOSS | levels_flag(5), a, 32) == 0 and es.check(AMBIENT_SH | levels_flag(1), a, 32) == 0
    assert es.check(AMBIENT_SH | levels_flag(2), a, 32) == 1 and es.check(AMBIENT_SH | levels_flag(5) | 1, a, 32) == 1
    assert es.check(AMBIENT_SH, 0, 32) == 2
    for mis in (1, 2, 3):
        assert es.check(AMBIENT_SH, a + mis, 32) == 3 and es.check(AMBIENT_SH | GLOSS | levels_flag(3), a + mis, 32) == 3
    assert es.check(AMBIENT_SH, a + 4, 32) == 0
    assert built_lib.LIGHT_AMBIENT_SH == AMBIENT_SH and built_lib.CUBE_SH_BYTES == TAIL_BYTES <= 1024
    from crychic_renderer_amd import geometry as g
    for dim, levels in ((1, 0), (1, 1), (2, 2), (5, 1), (5, 3), (20, 3), (32, 0), (32, 6), (256, 9), (8192, 14)):
        off = tail_offset(dim, levels)
        assert off % 16 == 0 and 0 <= off - int(lib.crychic_cube_chain_bytes(dim, max(levels, 1))) < 16
        assert int(lib.crychic_cube_sh_offset(dim, levels)) == off == es._host.eh_tail_offset(dim, levels) == es._ref.es_tail_offset(dim, levels)
        assert g.cube_sh_offset(dim, levels) == off and g.cube_chain_sh_bytes(dim, levels) == off + TAIL_BYTES
        assert int(lib.crychic_cube_chain_sh_bytes(dim, levels)) == off + TAIL_BYTES
    assert tail_offset(5, 1) == 608 and tail_offset(1, 1) == 32          # 600 and 24 rounded up
    # without a device the entry refuses NULL pointers before it looks for one
    assert lib.crychic_project_cube_sh(None, None, 4, None, None) != 0
