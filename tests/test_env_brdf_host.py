"""CPU tier of the split-sum specular term (include/crychic_hip.h "environment BRDF table"): the bodies of
env_brdf.hip and of the SpecularSplitSum lighting kernels, built for the host (tests/env_brdf_host), against the checker
(tests/env_brdf_ref) bit for bit; the properties of the definition; a float64 restatement and known answers; the tie to the frozen
gloss checker; the binding's refusals and the size functions."""
import ctypes as C

import numpy as np
import pytest

import env_brdf_lib
import env_sh_lib
import gloss_lib
from env_brdf_lib import ENV_BRDF, TABLE_BYTES, TAIL_BYTES, table_offset, with_table
from env_sh_lib import AMBIENT_SH
from test_env_sh_host import scene_block, with_edge_normals
from test_gloss_host import GLOSS, SIZES, edge_roughness, gloss_chain, levels_flag, same_frame

KNOWN = {(0, 31): (65239, 0), (0, 0): (669, 1744), (31, 31): (20744, 3), (31, 0): (38693, 1258), (15, 15): (37788, 573), (3, 0): (11815, 5281)}


@pytest.fixture(scope="module")
def eb():
    return env_brdf_lib.load()


@pytest.fixture(scope="module")
def es():
    return env_sh_lib.load()


@pytest.fixture(scope="module")
def gl():
    return gloss_lib.load()


def halves(table):
    t = np.asarray(table, np.uint32)
    return (t & 0xFFFF).astype(np.int64), (t >> 16).astype(np.int64)


# ---- the table -------------------------------------------------------------------------------------------------------------------------

def test_host_body_equals_the_checker_bit_for_bit(eb):
    """The 1024 dwords and the 2048 sums, whatever the destination held."""
    ref, sums = eb.table()
    for fill in (0xFF, 0x00, 0xA5):
        got, gsums = eb.host_table(fill)
        assert np.array_equal(got, ref) and np.array_equal(gsums, sums), fill


def test_the_sums_do_not_depend_on_how_the_samples_are_grouped(eb):
    """Any split of the 4096 samples into subsets, in any order, gives the same sums: the checker's by sample ranges, the body's by
    permuted and partitioned xi rows."""
    _, sums = eb.table()
    rng = np.random.default_rng(5)
    for j, i in ((0, 0), (0, 31), (3, 0), (15, 15), (31, 0), (31, 31), (7, 20)):
        whole = sums[j * 32 + i]
        for cut in (0, 1, 15, 16, 17, 1365, 2049, 4095, 4096):
            a, wa = eb.ref_sums(j, i, 0, cut)
            b, wb = eb.ref_sums(j, i, cut, 4096)
            assert np.array_equal(a + b, whole) and wa >= 0.0 and wb >= 0.0
        rows = rng.permutation(256)
        assert np.array_equal(eb.host_sums(j, i, rows), whole)
        parts = np.array_split(rows, [3, 64, 65, 200])
        assert np.array_equal(sum(eb.host_sums(j, i, part) for part in parts), whole)
        assert np.array_equal(eb.host_sums(j, i, np.arange(255, -1, -1)), whole)


def test_the_checker_asserts_the_bounds_of_the_definition(eb):
    """eb_table returns 0 only if every term lies in [0, 64), A + B <= 1 and B <= 0.15 on every texel; the figures of the definition
    (terms below 19.5, |S| < 2^42, the ranges of A and B) are printed and hold as well."""
    table, sums = eb.table()
    A, B = halves(table)
    worst = max(eb.ref_sums(j, i)[1] for j in range(32) for i in range(32))
    print("largest term %.4f; A in [%.4f, %.4f], B in [%.3g, %.4f], max A + B %.5f" %
          (worst, A.min() / 65535, A.max() / 65535, B.min() / 65535, B.max() / 65535, (A + B).max() / 65535))
    assert 0.0 < worst < 19.5 and np.abs(sums).max() < 2 ** 42 and sums.min() >= 0
    assert (A + B).max() <= 65535 and B.max() <= 9830
    # the definition's figures, to the places it states them with: A in [0.0102, 0.9955], B's upper end 0.1441 (its lower end, 3.9e-8,
    # is 0 units of R16) and max(A + B) = 0.99548
    assert round(A.min() / 65535, 4) == 0.0102 and round(A.max() / 65535, 4) == 0.9955
    assert B.min() == 0 and round(B.max() / 65535, 4) == 0.1441 and round((A + B).max() / 65535, 5) == 0.99548
    # B's lower end before the R16 quantisation: the float64 figure 3.9e-8, up to the per-term quantisation of 2^-25
    assert sums[:, 1].min() > 0 and abs(sums[:, 1].min() / 2.0 ** 36 - 3.9e-8) <= 2.0 ** -25


def _np_table():
    """The same quadrature in float64, written without the checker's helpers: (A, B) as (32, 32) arrays of R16 values."""
    j = np.arange(32, dtype=np.float64)[:, None, None, None]
    i = np.arange(32, dtype=np.float64)[None, :, None, None]
    rho, mu = (j + 0.5) / 32.0, (i + 0.5) / 32.0
    xi = ((np.arange(256) + 0.5) / 256.0)[None, None, :, None]
    cos_phi = np.cos(np.pi * (np.arange(16) + 0.5) / 16.0)[None, None, None, :]
    k = (rho + 1.0) ** 2 / 8.0
    vz, vx = mu, np.sqrt(1.0 - mu * mu)
    c2 = (1.0 - xi) / (1.0 + (rho * rho - 1.0) * xi)
    c, sn = np.sqrt(c2), np.sqrt(1.0 - c2)
    voh = vx * sn * cos_phi + vz * c
    lz = 2.0 * voh * c - vz
    above = lz > 0.0
    safe = np.where(above, lz, 1.0)
    g = (1.0 / (vz * (1.0 - k) + k)) * (safe / (safe * (1.0 - k) + k)) * voh / c
    fc = (1.0 - np.clip(voh, 0.0, 1.0)) ** 5
    A = np.where(above, (1.0 - fc) * g, 0.0).mean(axis=(2, 3))
    B = np.where(above, fc * g, 0.0).mean(axis=(2, 3))
    q = lambda x: np.floor(np.clip(x, 0.0, 1.0) * 65535.0 + 0.5).astype(np.int64)
    return q(A), q(B)


def test_float64_restatement_within_one_unit_of_r16(eb):
    """Every entry within 1 unit of R16 of the float64 run: an fp32 term is within a few 1e-6 relative of the real one and terms are
    <= 19.5 before the division by 4096, the quantisation adds <= 2^-25 per term -- together under 0.1 unit, plus one rounding
    boundary.  The sixteen cosine constants are the correctly rounded cosines."""
    A, B = halves(eb.table()[0])
    nA, nB = _np_table()
    dA, dB = np.abs(A.reshape(32, 32) - nA), np.abs(B.reshape(32, 32) - nB)
    print("largest difference: A %d, B %d units of R16; texels that differ: %d, %d" % (dA.max(), dB.max(), (dA > 0).sum(), (dB > 0).sum()))
    assert dA.max() <= 1 and dB.max() <= 1
    bits = [0x3f7ec46d, 0x3f74fa0b, 0x3f61c598, 0x3f45e403, 0x3f226799, 0x3ef15aea, 0x3e94a031, 0x3dc8bd36]
    want = np.cos(np.pi * (np.arange(8) + 0.5) / 16.0).astype(np.float32).view(np.uint32)
    assert list(want) == bits


def test_known_answers(eb):
    """Six entries of a float64 run of the definition, as (row j, column i) -> A, B, each within 1 unit."""
    A, B = halves(eb.table()[0])
    for (j, i), (a, b) in KNOWN.items():
        assert abs(int(A[j * 32 + i]) - a) <= 1 and abs(int(B[j * 32 + i]) - b) <= 1, ((j, i), A[j * 32 + i], B[j * 32 + i])


def test_lookup_at_texel_centres_and_outside(eb):
    """The bilinear lookup returns a texel at its centre, clamps outside the table and takes NaN for 0."""
    table = eb.table()[0]
    dec = lambda v: np.float32(v) / np.float32(65535.0)
    for j, i in ((0, 0), (31, 31), (7, 20), (31, 0)):
        ab = eb.lookup(table, (i + 0.5) / 32.0, (j + 0.5) / 32.0)
        assert ab[0] == dec(table[j * 32 + i] & 0xFFFF) and ab[1] == dec(table[j * 32 + i] >> 16)
    corner = eb.lookup(table, 0.0, 0.0)
    for u, v in ((-3.0, -1.0), (np.nan, np.nan), (-0.0, np.nan), (-np.inf, 0.0)):
        assert np.array_equal(eb.lookup(table, u, v), corner)
    assert np.array_equal(eb.lookup(table, 7.0, np.inf), eb.lookup(table, 1.0, 1.0))


# ---- the lighting pass -------------------------------------------------------------------------------------------------------------

def table_roughness():
    """0 and 1, every j / 32 and (j + 0.5) / 32 and one ulp either side, values < 0 and > 1, -0, +-inf and NaN."""
    v = [0.0, 1.0, -0.0, -0.5, -1e30, 1.5, 3e38, np.nan, -np.inf, np.inf]
    for j in range(33):
        for x in (np.float32(j / 32.0), np.float32((j + 0.5) / 32.0)):
            v += [x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2))]
    return np.array(v, np.float32)


def with_table_roughness(p, levels, shift=0):
    """The table's roughness edge values, and the gloss lookup's for `levels`, cycling through G1.w."""
    g1 = p["g1"].copy()
    v = np.concatenate([table_roughness(), edge_roughness(levels)])
    H, W = g1.shape[:2]
    g1[..., 3] = v[(np.arange(H)[:, None] * 11 + np.arange(W)[None, :] + shift) % len(v)]
    return dict(p, g1=g1)


def with_view_normals(p, eye):
    """On every fifth pixel a normal built from the pixel's own view vector: along it (N.V = 1 up to rounding), against it (negative),
    perpendicular to it (N.V about 0, either sign), and the unnormalised vector to the eye itself; test_env_sh_host's edge normals
    (zero-length, NaN, infinite, tiny) on every third of the others."""
    q = with_edge_normals(p)
    g2 = q["g2"].copy()
    H, W = g2.shape[:2]
    to_eye = (np.asarray(eye, np.float32)[None, None, :] - p["g0"][..., :3]).astype(np.float32)
    n = to_eye / np.maximum(np.linalg.norm(to_eye, axis=-1, keepdims=True), 1e-20).astype(np.float32)
    perp = np.stack([n[..., 1], -n[..., 0], np.zeros_like(n[..., 0])], -1)
    k = np.arange(H)[:, None] * 3 + np.arange(W)[None, :]
    for m, vec in enumerate((n, -n, perp, to_eye, -perp)):
        sel = (k % 5 == 0) & ((k // 5) % 5 == m)
        g2[..., :3][sel] = vec[sel]
    return dict(q, g2=g2)


def eye_of(cb):
    return [cb.EyePosW[0], cb.EyePosW[1], cb.EyePosW[2]]


def with_eye(cb, eye):
    """(a copy of the ctypes pass constants with EyePosW = eye, the oracle's view of it)"""
    import oracle_lib
    c2 = type(cb).from_buffer_copy(cb)
    c2.EyePosW[:] = list(eye)
    return c2, oracle_lib.as_oracle_cb(c2, oracle_lib.OrPassConstants)


def random_table(seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, 1024, dtype=np.uint64).astype(np.uint32)


def spec_flags(levels, sh=False):
    return ENV_BRDF | GLOSS | levels_flag(levels) | (AMBIENT_SH if sh else 0)


@pytest.mark.parametrize("levels", [2, 5])
@pytest.mark.parametrize("W,H", SIZES)
def test_spec_body_matches_checker_without_local_lights(built_lib, eb, es, gl, W, H, levels):
    """The host body == the checker, RGBA8 and radiance bits: the built table and tables of random dwords, the roughness and normal edge
    values, with and without SH, both PCF radii, Q fixes off and on, sky on and off, and an infinite EyePosW."""
    from local_lights_util import FIX_ALL, _cpu
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, levels)
    block = scene_block(es, p)
    for k, table in enumerate((eb.table()[0], random_table(levels), random_table(100 + W))):
        q = with_view_normals(with_table_roughness(p, levels, shift=k), eye_of(c.pass_cb))
        qq = dict(q, cube=with_table(chain, dim, levels, table, block))
        for sh in (False, True):
            fixes, ndl, radius, sky = ((0, 1, 0.0, 1), (FIX_ALL, 3, 2.5 / 256, 0))[(k + sh) & 1]
            flags = fixes | sky | spec_flags(levels, sh)
            got = eb.host_light(c.pass_cb, qq, None, ndl, radius, flags, cube_dim=dim)
            ref = eb.checker_light(pcb, qq, None, ndl, radius, flags, cube_dim=dim)
            assert same_frame(got, ref), (levels, k, sh)
    cb2, pcb2 = with_eye(c.pass_cb, (np.inf, 3.0, -np.inf))
    for sh in (False, True):
        got = eb.host_light(cb2, qq, None, 3, 0.0, 1 | spec_flags(levels, sh), cube_dim=dim)
        assert same_frame(got, eb.checker_light(pcb2, qq, None, 3, 0.0, 1 | spec_flags(levels, sh), cube_dim=dim)), sh
    lit = (p["depth"] & 0xFFFFFF) < 0xFFFFFF
    assert lit.any() and (~lit).any()


@pytest.mark.parametrize("levels", [2, 5])
def test_spec_body_matches_checker_with_local_lights_and_shadows(built_lib, eb, es, gl, levels):
    """Points, spots, 3 shadowed spots and 2 shadowed points; then the same without any shadow; both sizes, both radii, without and with
    SH."""
    from local_lights_util import FIX_ALL
    from test_point_shadows import _frame_setup
    for (W, H), radius, fixes, sh in zip(SIZES, (0.0, 0.01), (0, FIX_ALL), (False, True)):
        p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, 2, 48, 3, seed=3 + levels)
        chain, dim = gloss_chain(gl, p, levels)
        q = dict(with_view_normals(with_table_roughness(p, levels), eye_of(cb)),
                 cube=with_table(chain, dim, levels, eb.table()[0], scene_block(es, p)))
        flags = fixes | 1 | spec_flags(levels, sh)
        for args in (dict(points=points, spots=spots, maps=maps, cubes=cubes, projs=projs), dict(points=points, spots=spots), dict(points=points)):
            got = eb.host_light(cb, q, None, 3, radius, flags, cube_dim=dim, **args)
            ref = eb.checker_light(pcb, q, None, 3, radius, flags, cube_dim=dim, **args)
            assert same_frame(got, ref), (W, H, levels, sorted(args))


def test_spec_body_matches_checker_on_a_half_float_mix_and_with_an_ambient_map(built_lib, eb, es, gl):
    """G0 float4 with G1 and G2 half4: the body on the packed planes == the checker on the widened planes; then float planes with a
    half-res ambient map (ambientAccess != 1)."""
    import gbuffer_f16_lib as gf
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    for levels, sh in ((2, True), (5, False)):
        chain, dim = gloss_chain(gl, p, levels)
        q = dict(with_view_normals(with_table_roughness(p, levels), eye_of(c.pass_cb)),
                 cube=with_table(chain, dim, levels, eb.table()[0], scene_block(es, p)))
        packed = gf.pack_planes(q, gf.MIXED)
        wide = gf.widen_planes(packed)
        flags = 1 | spec_flags(levels, sh)
        got = eb.host_light(c.pass_cb, packed, None, 3, 0.0, flags, cube_dim=dim, formats=True)
        assert same_frame(got, eb.checker_light(pcb, wide, None, 3, 0.0, flags, cube_dim=dim))
        ao = np.random.default_rng(levels).integers(0, 65536, (H // 2, W // 2), dtype=np.uint16)
        got = eb.host_light(c.pass_cb, q, ao, 3, 0.01, flags, cube_dim=dim)
        assert same_frame(got, eb.checker_light(pcb, q, ao, 3, 0.01, flags, cube_dim=dim))


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_spec_fuzz_planes_through_checker_and_body(built_lib, eb, es, seed):
    """fuzz_util's planes (NaN, inf, zero-length vectors) with the flag set, the box chain taken as a gloss chain, a random table."""
    import fuzz_util
    import oracle_lib
    from crychic_renderer_amd import geometry as g
    W, H, planes, c, knobs = fuzz_util.random_case(seed, built_lib)
    chain, levels = g.cube_mip_chain(planes["cube"])
    dim = planes["cube"].shape[1]
    assert levels > 1
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    block = es.project(planes["cube"])
    for sh, table in ((False, eb.table()[0]), (True, random_table(seed))):
        q = dict(planes, cube=with_table(chain, dim, levels, table, block))
        flags = knobs["sky"] | spec_flags(levels, sh)
        got = eb.host_light(c.pass_cb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)
        ref = eb.checker_light(pcb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)
        assert same_frame(got, ref), sh


# ---- the tie to the old path -----------------------------------------------------------------------------------------------------------

def test_a_table_of_b_equal_one_is_the_frozen_gloss_frame_of_a_white_mirror_metal(built_lib, eb, gl):
    """A = 0, B = 1 on every texel, roughness 0, metalness 1, albedo 1: R0 == 1.0f exactly, so the old weight is shininess *
    fma(1 - R0, f5, R0) = 1 * fma(0, f5, 1) = 1 and the new one fma(R0, 0, 1) = 1 -- the flagged frame, checker and host body, is the
    frozen gloss checker's frame bit for bit."""
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    g0, g1 = p["g0"].copy(), p["g1"].copy()
    g0[..., 3] = 1.0
    g1[...] = (1.0, 1.0, 1.0, 0.0)
    assert np.array_equal(eb.r0([1.0, 1.0, 1.0], 1.0), np.ones(3, np.float32))
    q = dict(p, g0=g0, g1=g1)
    ones = np.full(1024, 0xFFFF0000, np.uint32)
    for levels in (2, 5):
        chain, dim = gloss_chain(gl, p, levels)
        base = gl.checker_light(pcb, dict(q, cube=chain), None, 3, 0.0, 1 | GLOSS | levels_flag(levels), cube_dim=dim)
        qq = dict(q, cube=with_table(chain, dim, levels, ones))
        for fn, cb in ((eb.checker_light, pcb), (eb.host_light, c.pass_cb)):
            assert same_frame(fn(cb, qq, None, 3, 0.0, 1 | spec_flags(levels), cube_dim=dim), base), levels
        # ... and the built table gives another frame: the flag bites
        other = eb.checker_light(pcb, dict(q, cube=with_table(chain, dim, levels, eb.table()[0])), None, 3, 0.0, 1 | spec_flags(levels), cube_dim=dim)
        assert (other[0] != base[0]).any()


def test_a_table_of_zeros_is_the_gloss_frame_over_a_black_chain(built_lib, eb, gl):
    """A = B = 0: spec = fma(R0, 0, 0) = 0 and the reflection adds nothing, as it adds nothing in the gloss frame whose chain holds
    colour 0 everywhere (sky off: the sky reads the chain)."""
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, pcb = _cpu(W, H)
    levels = 5
    chain, dim = gloss_chain(gl, p, levels)
    black = np.zeros_like(chain)
    black[3::4] = 255
    base = gl.checker_light(pcb, dict(p, cube=black), None, 3, 0.0, GLOSS | levels_flag(levels), cube_dim=dim)
    qq = dict(p, cube=with_table(chain, dim, levels, np.zeros(1024, np.uint32)))
    for fn, cb in ((eb.checker_light, pcb), (eb.host_light, c.pass_cb)):
        assert same_frame(fn(cb, qq, None, 3, 0.0, spec_flags(levels), cube_dim=dim), base)
    lit = gl.checker_light(pcb, dict(p, cube=chain), None, 3, 0.0, GLOSS | levels_flag(levels), cube_dim=dim)
    assert (lit[0] != base[0]).any()


# ---- refusals and size functions ---------------------------------------------------------------------------------------------------------

def test_refusals_of_the_binding_and_the_size_functions(built_lib, eb):
    """The flag without a gloss chain, with a null cube map and with a misaligned table is refused by light_bind.hpp's check, each with
    the message the entries report; the host body refuses the same; the size functions of the library, the harness and the checker
    agree."""
    lib = built_lib.lib
    a = 0x10000
    ok = ENV_BRDF | GLOSS | levels_flag(5)
    assert eb.check(ok, a, 32) == 0 and eb.check(0, 0, 32) == 0 and eb.check(ok | AMBIENT_SH, a, 32) == 0
    assert eb.check(ENV_BRDF | GLOSS | levels_flag(2), a, 32) == 0
    for bad in (ENV_BRDF, ENV_BRDF | levels_flag(5), ENV_BRDF | GLOSS, ENV_BRDF | GLOSS | levels_flag(1), ENV_BRDF | AMBIENT_SH,
                ENV_BRDF | levels_flag(1)):
        assert eb.check(bad, a, 32) == 1, hex(bad)
    assert eb.check(ok, 0, 32) == 2
    for mis in (1, 2, 3):
        assert eb.check(ok, a + mis, 32) == 3
    assert eb.check(ok, a + 4, 32) == 0
    assert eb.check_message(ok, a, 32) == "" and eb.check_message(0, 0, 32) == ""
    assert eb.check_message(ENV_BRDF | levels_flag(5), a, 32) == eb.check_message(ENV_BRDF | GLOSS, a, 32) == \
        "CRYCHIC_LIGHT_ENV_BRDF needs a prefiltered chain: CRYCHIC_LIGHT_CUBE_LEVELS(n) with n > 1 and CRYCHIC_LIGHT_CUBE_GLOSS"
    assert eb.check_message(ok, 0, 32) == "CRYCHIC_LIGHT_ENV_BRDF: null cube map"
    assert eb.check_message(ok, a + 2, 32) == "CRYCHIC_LIGHT_ENV_BRDF: the table at cube_dev + %d is not 4-byte aligned" % table_offset(32, 5)
    assert built_lib.LIGHT_ENV_BRDF == ENV_BRDF == 0x100000 and built_lib.ENV_BRDF_BYTES == TABLE_BYTES == 4096
    assert ENV_BRDF & (0xF0000 | 0xFFFF) == 0            # clear of the level count and of every other flag
    from crychic_renderer_amd import geometry as g
    for dim, levels in ((1, 0), (1, 1), (2, 2), (5, 1), (5, 3), (20, 3), (32, 0), (32, 6), (256, 9), (8192, 14)):
        off = table_offset(dim, levels)
        assert off == int(lib.crychic_cube_sh_offset(dim, levels)) + TAIL_BYTES and off % 16 == 0
        assert int(lib.crychic_cube_env_brdf_offset(dim, levels)) == off == eb._host.bh_table_offset(dim, levels) == eb._ref.eb_table_offset(dim, levels)
        assert g.cube_env_brdf_offset(dim, levels) == off and g.cube_chain_env_bytes(dim, levels) == off + TABLE_BYTES
        assert int(lib.crychic_cube_chain_env_bytes(dim, levels)) == off + TABLE_BYTES
    assert table_offset(5, 1) == 608 + 512 and table_offset(1, 1) == 32 + 512
    # without a device the entry refuses a NULL context before it looks for one
    assert lib.crychic_build_env_brdf(None, None, None) != 0


def test_host_body_refuses_what_the_entries_refuse(built_lib, eb, gl):
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, _ = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, 2)
    q = dict(p, cube=with_table(chain, dim, 2, eb.table()[0]))
    from hostsim_lib import run_light
    rcs = []

    class Rec:          # run_light discards the entry point's return value: a recording wrapper keeps it
        argtypes = eb._host.bh_light.argtypes
        def __call__(self, *a):
            rcs.append(eb._host.bh_light(*a))
    for flags in (ENV_BRDF | levels_flag(2), ENV_BRDF | GLOSS, ENV_BRDF | GLOSS | levels_flag(2)):
        run_light(Rec(), c.pass_cb, q, None, 1, 0.0, flags, cube_dim=dim)
    assert rcs == [-1, -1, 0]
