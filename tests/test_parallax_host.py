"""CPU tier of the box-projected reflection lookup (include/crychic_hip.h "probe volume"): light_core.hpp's
probe_project and the CubeGlossBox lighting kernels' bodies, built for the host (tests/parallax_host), against the checker
(tests/parallax_ref) bit for bit; the known answers of the definition; a frame on which the flag bites; the binding's refusals,
the setter's argument check and the size function; and the frames without the flag, which stay what they were."""
import os

import numpy as np
import pytest

import env_brdf_lib
import env_sh_lib
import gloss_lib
import parallax_lib
from env_brdf_lib import ENV_BRDF
from env_sh_lib import AMBIENT_SH
from parallax_lib import PARALLAX, PROBE_BYTES, PROBE_OFFSET, probe_floats, probe_offset, with_probe
from test_env_brdf_host import eye_of, random_table, with_table_roughness, with_view_normals
from test_env_sh_host import scene_block
from test_gloss_host import GLOSS, SIZES, gloss_chain, levels_flag, same_frame

BOX = ((0.0, 0.0, 0.0), (-4.0, -2.0, -4.0), (4.0, 6.0, 4.0))        # the definition's known answers: c, bmin, bmax
COMBOS = [(False, False), (True, False), (False, True), (True, True)]      # (SH ambient, split sum)


@pytest.fixture(scope="module")
def px():
    return parallax_lib.load()


@pytest.fixture(scope="module")
def eb():
    return env_brdf_lib.load()


@pytest.fixture(scope="module")
def es():
    return env_sh_lib.load()


@pytest.fixture(scope="module")
def gl():
    return gloss_lib.load()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box_flags(levels, sh=False, spec=False):
    return PARALLAX | GLOSS | levels_flag(levels) | (AMBIENT_SH if sh else 0) | (ENV_BRDF if spec else 0)


# ---- the correction ----------------------------------------------------------------------------------------------------------------------

def test_known_answers_through_checker_and_body(px):
    """The four rows of the definition's table, and more derived by hand (all exact in binary32): a ray leaving through -X, through the
    top, one starting outside the box beyond the face it heads for (t clamps to 0), a subnormal component skipped, a NaN component
    skipped, an infinite component (rcp gives 0, so t_k = 0 and the hit is NaN = inf * 0 on that axis), and a capture position off the
    origin."""
    inf, nan = np.inf, np.nan
    probe = probe_floats(*BOX)
    cases = [
        ((1, -2, 1), (0.5, 0.5, 0), 6.0, (4, 1, 1)),
        ((1, -2, 1), (0.5, 0.5, -0.0), 6.0, (4, 1, 1)),
        ((1, -2, 1), (0, 0, 0), inf, (0, 0, 0)),
        ((1, -2.5, 1), (0, -1, 0), 0.0, (1, -2.5, 1)),
        ((1, 0, 0), (-0.5, 0.25, 0), 10.0, (-4, 2.5, 0)),                  # -X: t_x = (-4 - 1) / -0.5 = 10, t_y = 6 / 0.25 = 24
        ((0, 2, 0), (0, 2, 0.5), 2.0, (0, 6, 1)),                          # the top: t_y = 4 / 2 = 2, t_z = 4 / 0.5 = 8
        ((5, 0, 0), (1, 0, 0), 0.0, (5, 0, 0)),                            # outside, beyond +X: e = -1, t = -1 -> 0
        ((1, -2, 1), (0.5, 0.5, 1e-40), 6.0, (4, 1, 1 + 6e-40)),           # a subnormal component: skipped; fma(r_z, 6, 1) rounds to 1
        ((1, -2, 1), (0.5, nan, 0), 6.0, (4, nan, 1)),                     # a NaN component: skipped, and h_y = fma(NaN, ..) is NaN
        ((0, 0, 0), (inf, 1, 0), 0.0, (nan, 0, 0)),                        # rcp(inf) = 0: t_x = 4 * 0 = 0; h_x = fma(inf, 0, 0) = NaN
    ]
    p = np.array([c[0] for c in cases], np.float32)
    r = np.array([c[1] for c in cases], np.float32)
    want = np.array([c[3] for c in cases], np.float32)
    got, t = px.ref_correct(p, r, np.tile(probe, (len(cases), 1)))
    body = px.host_correct(p, r, np.tile(probe, (len(cases), 1)))
    for k, c in enumerate(cases):
        assert t[k] == np.float32(c[2]), (k, t[k])
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, got[k])
    assert np.array_equal(bits(body)[~np.isnan(body)], bits(got)[~np.isnan(got)]) and np.array_equal(np.isnan(body), np.isnan(got))
    assert np.array_equal(bits(got[1]), bits(got[0]))          # the zero component is skipped whatever its sign
    assert np.array_equal(bits(got[2]), bits(r[2]))            # r' = r: the very bits
    # a capture position off the origin moves r' and nothing else
    off = probe_floats((1.0, 0.5, -2.0), BOX[1], BOX[2])
    g2, t2 = px.ref_correct(p[:1], r[:1], off[None])
    assert t2[0] == 6.0 and np.array_equal(g2[0], np.array([3.0, 0.5, 3.0], np.float32))


SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38, 1.1754942e-38, np.inf, -np.inf, np.nan, 3e38, -3e38, 1e-30], np.float32)


def random_triples(seed, n):
    """(p, r, probe): boxes of every size around capture positions anywhere; p inside, outside, and exactly on each face; r of every
    length; and +-0, subnormals, the smallest normal and the largest subnormal, +-inf, NaN and huge values in components of r and p."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-20, 20, (n, 3))
    lo = c - rng.uniform(0.01, 30, (n, 3)) ** rng.choice([1.0, 0.3, 2.0], (n, 1))
    hi = c + rng.uniform(0.01, 30, (n, 3)) ** rng.choice([1.0, 0.3, 2.0], (n, 1))
    p = lo + (hi - lo) * rng.uniform(-0.5, 1.5, (n, 3))
    r = rng.normal(0, 1, (n, 3)) * 10.0 ** rng.integers(-3, 3, (n, 1))
    p, r, lo, hi, c = (a.astype(np.float32) for a in (p, r, lo, hi, c))
    k = np.arange(n)
    for axis in range(3):                                   # exactly on a face, and one ulp either side of it
        on = (k % 7 == axis)
        face = np.where(rng.random(n) < 0.5, lo[:, axis], hi[:, axis])
        nudge = rng.integers(-1, 2, n)
        moved = np.where(nudge < 0, np.nextafter(face, np.float32(-np.inf)), np.where(nudge > 0, np.nextafter(face, np.float32(np.inf)), face))
        p[on, axis] = moved[on]
    for a, every in ((r, 3), (p, 11)):
        sel = rng.random((n, 3)) < 1.0 / every
        a[sel] = SPECIAL[rng.integers(0, len(SPECIAL), int(sel.sum()))]
    r[k % 13 == 0] = 0.0
    probe = np.zeros((n, 12), np.float32)
    probe[:, 0:3], probe[:, 4:7], probe[:, 8:11] = c, lo, hi
    return p, r, probe


def test_ten_thousand_random_triples_checker_equals_body(px):
    p, r, probe = random_triples(18, 10000)
    ref, t = px.ref_correct(p, r, probe)
    got = px.host_correct(p, r, probe)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(got))
    assert np.array_equal(bits(ref)[~nan], bits(got)[~nan])
    # the cases the definition names all occur: nothing usable, the clamp, every axis as the exit, non-finite results
    unusable = ~(t < np.inf)
    assert unusable.sum() > 100 and np.array_equal(bits(ref[unusable])[~nan[unusable]], bits(r[unusable])[~nan[unusable]])
    assert (t == 0).sum() > 100 and ((t > 0) & (t < np.inf)).sum() > 1000 and nan.any() and np.isinf(ref).any()


# ---- frames ------------------------------------------------------------------------------------------------------------------------------

def scene_probe(k=0):
    """Probe volumes around the CPU scene: one that holds most of it, one that most positions lie outside of, one off centre."""
    return [probe_floats((0.0, 3.0, 0.0), (-25.0, -1.0, -25.0), (25.0, 18.0, 25.0)),
            probe_floats((1.0, 1.0, -2.0), (-2.0, 0.5, -6.0), (3.0, 2.0, 1.0)),
            probe_floats((-7.5, 4.0, 9.0), (-30.0, 0.0, -12.0), (-1.0, 9.0, 40.0))][k % 3]


@pytest.mark.parametrize("levels", [2, 5])
@pytest.mark.parametrize("W,H", SIZES)
def test_box_body_matches_checker_without_local_lights(built_lib, px, eb, es, gl, W, H, levels):
    """The host body == the checker, RGBA8 and radiance bits, over the four ambient x specular combinations: the roughness and normal
    edge values, both PCF radii, Q fixes off and on, sky on and off, three probe volumes, and an infinite EyePosW."""
    from local_lights_util import FIX_ALL, _cpu
    from test_env_brdf_host import with_eye
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, levels)
    block = scene_block(es, p)
    q = with_view_normals(with_table_roughness(p, levels), eye_of(c.pass_cb))
    for k, (sh, spec) in enumerate(COMBOS):
        qq = dict(q, cube=with_probe(chain, dim, levels, scene_probe(k + levels), block, eb.table()[0] if spec else None))
        fixes, ndl, radius, sky = ((0, 1, 0.0, 1), (FIX_ALL, 3, 2.5 / 256, 0))[k & 1]
        flags = fixes | sky | box_flags(levels, sh, spec)
        got = px.host_light(c.pass_cb, qq, None, ndl, radius, flags, cube_dim=dim)
        ref = px.checker_light(pcb, qq, None, ndl, radius, flags, cube_dim=dim)
        assert same_frame(got, ref), (levels, sh, spec)
    cb2, pcb2 = with_eye(c.pass_cb, (np.inf, 3.0, -np.inf))
    flags = 1 | box_flags(levels, True, True)
    assert same_frame(px.host_light(cb2, qq, None, 3, 0.0, flags, cube_dim=dim), px.checker_light(pcb2, qq, None, 3, 0.0, flags, cube_dim=dim))
    lit = (p["depth"] & 0xFFFFFF) < 0xFFFFFF
    assert lit.any() and (~lit).any()


@pytest.mark.parametrize("levels", [2, 5])
def test_box_body_matches_checker_with_local_lights_and_shadows(built_lib, px, eb, es, gl, levels):
    """Points, spots, 3 shadowed spots and 2 shadowed points; then without any shadow; then points alone: both sizes, both radii, the
    four combinations."""
    from local_lights_util import FIX_ALL
    from test_point_shadows import _frame_setup
    for n, ((W, H), radius, fixes) in enumerate(zip(SIZES, (0.0, 0.01), (0, FIX_ALL))):
        p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, 2, 48, 3, seed=3 + levels)
        chain, dim = gloss_chain(gl, p, levels)
        q = with_view_normals(with_table_roughness(p, levels), eye_of(cb))
        block = scene_block(es, p)
        for k, (sh, spec) in enumerate(COMBOS):
            qq = dict(q, cube=with_probe(chain, dim, levels, scene_probe(k + n), block, eb.table()[0] if spec else None))
            flags = fixes | 1 | box_flags(levels, sh, spec)
            args = (dict(points=points, spots=spots, maps=maps, cubes=cubes, projs=projs), dict(points=points, spots=spots), dict(points=points))[(k + n) % 3]
            got = px.host_light(cb, qq, None, 3, radius, flags, cube_dim=dim, **args)
            ref = px.checker_light(pcb, qq, None, 3, radius, flags, cube_dim=dim, **args)
            assert same_frame(got, ref), (W, H, levels, sh, spec, sorted(args))


def test_box_body_matches_checker_on_a_half_float_mix_and_with_an_ambient_map(built_lib, px, eb, es, gl):
    """G0 float4 with G1 and G2 half4: the body on the packed planes == the checker on the widened planes, frame and local-light
    shapes; then float planes with a half-res ambient map (ambientAccess != 1)."""
    import gbuffer_f16_lib as gf
    from local_lights_util import _cpu, points_for_test
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    points = points_for_test()
    for n, (levels, (sh, spec)) in enumerate(zip((2, 5, 5, 2), COMBOS)):
        chain, dim = gloss_chain(gl, p, levels)
        q = dict(with_view_normals(with_table_roughness(p, levels), eye_of(c.pass_cb)),
                 cube=with_probe(chain, dim, levels, scene_probe(n), scene_block(es, p), eb.table()[0] if spec else None))
        packed = gf.pack_planes(q, gf.MIXED)
        wide = gf.widen_planes(packed)
        flags = 1 | box_flags(levels, sh, spec)
        args = dict(points=points) if n & 1 else {}
        got = px.host_light(c.pass_cb, packed, None, 3, 0.0, flags, cube_dim=dim, formats=True, **args)
        assert same_frame(got, px.checker_light(pcb, wide, None, 3, 0.0, flags, cube_dim=dim, **args)), n
        ao = np.random.default_rng(levels).integers(0, 65536, (H // 2, W // 2), dtype=np.uint16)
        got = px.host_light(c.pass_cb, q, ao, 3, 0.01, flags, cube_dim=dim, **args)
        assert same_frame(got, px.checker_light(pcb, q, ao, 3, 0.01, flags, cube_dim=dim, **args)), n


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_box_fuzz_planes_through_checker_and_body(built_lib, px, eb, es, seed):
    """tests/test_fuzz.py's generator (fuzz_util's planes: NaN, inf, zero-length vectors) with the flag set, the box chain taken as a
    gloss chain, every combination."""
    import fuzz_util
    import oracle_lib
    from crychic_renderer_amd import geometry as g
    W, H, planes, c, knobs = fuzz_util.random_case(seed, built_lib)
    chain, levels = g.cube_mip_chain(planes["cube"])
    dim = planes["cube"].shape[1]
    assert levels > 1
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    block = es.project(planes["cube"])
    for k, (sh, spec) in enumerate(COMBOS):
        q = dict(planes, cube=with_probe(chain, dim, levels, scene_probe(seed + k), block, random_table(seed) if spec else None))
        flags = knobs["sky"] | box_flags(levels, sh, spec)
        got = px.host_light(c.pass_cb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)
        ref = px.checker_light(pcb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)
        assert same_frame(got, ref), (sh, spec)


# ---- the feature bites -------------------------------------------------------------------------------------------------------------------

FACE_COLOURS = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255], [255, 255, 0, 255], [0, 255, 255, 255], [255, 0, 255, 255]], np.uint8)
BITES_DIM, BITES_LEVELS = 8, 4
BITES_PROBE = ((0.0, 1.0, 0.0), (-4.0, -1.0, -4.0), (4.0, 40.0, 4.0))


def face_chain(colours):
    """A chain of BITES_LEVELS levels at BITES_DIM in which face f of every level holds colours[f] on every texel."""
    parts = []
    for k in range(BITES_LEVELS):
        d = max(BITES_DIM >> k, 1)
        parts.append(np.repeat(np.asarray(colours, np.uint8)[:, None, :], d * d, axis=1).reshape(-1))
    return np.concatenate(parts)


def bites_frame():
    """(planes without a cube map, eye): 64 x 4 covered floor pixels at y = 0 with normal +Y, x from 3.5 up to 3.9 -- close to the +X face
    of BITES_PROBE's box -- roughness 0 (level 0), a half-metal grey; the eye high above the origin, so that r = (-view.x, view.y,
    -view.z) is mostly +Y and slightly +X.  t_x = (4 - x) / r_x is about 2.5 to 4 and t_y about 40: the ray leaves through +X at a height of
    about 2.5 to 4, so r' = hit - c has its largest component along +X."""
    from local_lights_util import _cpu
    _, p, c, _ = _cpu(64, 48)
    H, W = 4, 64
    g0 = np.zeros((H, W, 4), np.float32)
    g0[..., 0] = (3.5 + 0.4 * np.arange(W) / (W - 1))[None, :]
    g0[..., 2] = (0.25 * np.arange(H) - 0.375)[:, None]
    g0[..., 3] = 0.5
    g1 = np.zeros((H, W, 4), np.float32)
    g1[..., :3] = 0.5
    g2 = np.zeros((H, W, 4), np.float32)
    g2[..., 1] = 1.0
    planes = dict(g0=g0, g1=g1, g2=g2, depth=np.zeros((H, W), np.uint32), shadow=p["shadow"])
    return planes, c, (0.0, 30.0, 0.0)


def test_the_flag_moves_the_reflection_from_the_top_face_to_the_side_face(built_lib, px, gl):
    """Six distinct face colours.  Without the flag every pixel reflects the +Y face: the frozen gloss checker's frame over the real chain
    is its frame over a chain whose faces all have +Y's colour.  With the flag every pixel reflects the +X face: checker and body give
    the frame of the chain whose faces all have +X's colour -- and the two frames differ on every pixel."""
    from test_env_brdf_host import with_eye
    planes, c, eye = bites_frame()
    cb, pcb = with_eye(c.pass_cb, eye)
    probe = probe_floats(*BITES_PROBE)
    base = GLOSS | levels_flag(BITES_LEVELS)
    real = face_chain(FACE_COLOURS)
    all_x, all_y = face_chain(FACE_COLOURS[[0] * 6]), face_chain(FACE_COLOURS[[2] * 6])

    def cube(chain):
        return with_probe(chain, BITES_DIM, BITES_LEVELS, probe)
    without = gl.checker_light(pcb, dict(planes, cube=real), None, 1, 0.0, base, cube_dim=BITES_DIM)
    assert same_frame(without, gl.checker_light(pcb, dict(planes, cube=all_y), None, 1, 0.0, base, cube_dim=BITES_DIM))
    with_flag = px.checker_light(pcb, dict(planes, cube=cube(real)), None, 1, 0.0, base | PARALLAX, cube_dim=BITES_DIM)
    assert same_frame(with_flag, gl.checker_light(pcb, dict(planes, cube=all_x), None, 1, 0.0, base, cube_dim=BITES_DIM))
    body = px.host_light(cb, dict(planes, cube=cube(real)), None, 1, 0.0, base | PARALLAX, cube_dim=BITES_DIM)
    assert same_frame(body, with_flag)
    assert (with_flag[0] != without[0]).any(axis=-1).all()
    assert same_frame(px.host_light(cb, dict(planes, cube=cube(real)), None, 1, 0.0, base, cube_dim=BITES_DIM), without)


# ---- refusals, the setter's check, the size function -----------------------------------------------------------------------------------------

def test_refusals_of_the_binding_and_the_size_function(built_lib, px):
    """The flag without a gloss chain, with a null cube map and with a misaligned probe volume is refused by light_bind.hpp's check,
    each with the message the entries report -- api.cpp formats that very function's text; the size functions of the library, the
    harness and the checker agree."""
    lib = built_lib.lib
    a = 0x10000
    ok = box_flags(5)
    for sh, spec in COMBOS:
        assert px.check(box_flags(5, sh, spec), a, 32) == 0 and px.check(box_flags(2, sh, spec), a, 32) == 0
    assert px.check(0, 0, 32) == 0 and px.check(GLOSS | levels_flag(5), 0, 32) == 0
    for bad in (PARALLAX, PARALLAX | levels_flag(5), PARALLAX | GLOSS, PARALLAX | GLOSS | levels_flag(1), PARALLAX | AMBIENT_SH,
                PARALLAX | levels_flag(1), PARALLAX | AMBIENT_SH | levels_flag(1), PARALLAX | ENV_BRDF | levels_flag(5)):
        assert px.check(bad, a, 32) == 1, hex(bad)
    assert px.check(ok, 0, 32) == 2
    for mis in (1, 2, 3):
        assert px.check(ok, a + mis, 32) == 3
    assert px.check(ok, a + 4, 32) == 0
    assert px.check_message(ok, a, 32) == "" and px.check_message(0, 0, 32) == ""
    assert px.check_message(PARALLAX | levels_flag(5), a, 32) == px.check_message(PARALLAX | GLOSS, a, 32) == \
        "CRYCHIC_LIGHT_CUBE_PARALLAX needs a prefiltered chain: CRYCHIC_LIGHT_CUBE_LEVELS(n) with n > 1 and CRYCHIC_LIGHT_CUBE_GLOSS"
    assert px.check_message(ok, 0, 32) == "CRYCHIC_LIGHT_CUBE_PARALLAX: null cube map"
    assert px.check_message(ok, a + 2, 32) == "CRYCHIC_LIGHT_CUBE_PARALLAX: the probe volume at cube_dev + %d is not 4-byte aligned" % probe_offset(32, 5)
    # api.cpp states no text of its own for these refusals: it formats parallax_check_message with the probe volume's offset
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    api = open(os.path.join(root, "crychic_renderer_amd", "csrc", "api.cpp")).read()
    assert "fail(CRYCHIC_E_INVALID_ARG, cry::parallax_check_message(c), cry::parallax_probe_offset(cubeDim, (flags >> 16) & 15u))" in api
    # its definition and its one call, in check_environment; that one is defined once and called by both lighting paths
    assert api.count("check_parallax(") == 2 and api.count("check_environment(") == 3 and '"CRYCHIC_LIGHT_CUBE_PARALLAX' not in api
    assert built_lib.LIGHT_CUBE_PARALLAX == PARALLAX == 0x200000
    assert PARALLAX & (0xF0000 | 0xFFFF | ENV_BRDF) == 0          # clear of the level count and of every other flag
    from crychic_renderer_amd import geometry as g
    for dim, levels in ((1, 0), (1, 1), (2, 2), (5, 1), (5, 3), (20, 3), (32, 0), (32, 6), (256, 9), (8192, 14)):
        off = probe_offset(dim, levels)
        assert off == int(lib.crychic_cube_sh_offset(dim, levels)) + 368 and off % 16 == 0
        assert int(lib.crychic_cube_probe_offset(dim, levels)) == off == px._host.xh_probe_offset(dim, levels) == px._ref.px_probe_offset(dim, levels)
        assert g.cube_probe_offset(dim, levels) == off
        assert off + PROBE_BYTES <= int(lib.crychic_cube_chain_sh_bytes(dim, levels)) <= int(lib.crychic_cube_chain_env_bytes(dim, levels))
    assert (PROBE_OFFSET, PROBE_BYTES) == (368, 48) == (built_lib.CUBE_PROBE_OFFSET, built_lib.CUBE_PROBE_BYTES)
    assert probe_offset(5, 1) == 608 + 368 and probe_offset(1, 1) == 32 + 368
    # without a device the setter refuses a NULL context before it looks for one
    assert lib.crychic_set_cube_probe_volume(None, None, None, None, None, None) != 0


def test_the_setters_check_of_its_values(px):
    """Finite, and boxMin < pos < boxMax strictly in every component."""
    c, lo, hi = (np.array(v, np.float32) for v in BOX)
    assert px.volume_valid(c, lo, hi) and px.volume_valid((1, 0.5, -2), lo, hi)
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            for which in range(3):
                v = [c.copy(), lo.copy(), hi.copy()]
                v[which][k] = bad
                assert not px.volume_valid(*v), (k, bad, which)
        on_lo, on_hi, out = c.copy(), c.copy(), c.copy()
        on_lo[k], on_hi[k], out[k] = lo[k], hi[k], hi[k] + 1
        assert not px.volume_valid(on_lo, lo, hi) and not px.volume_valid(on_hi, lo, hi) and not px.volume_valid(out, lo, hi)
        flat = hi.copy()
        flat[k] = lo[k]
        assert not px.volume_valid(c, lo, flat) and not px.volume_valid(c, hi, lo)
        inside = c.copy()
        inside[k] = np.nextafter(lo[k], np.float32(np.inf))
        assert px.volume_valid(inside, lo, hi)


def test_the_three_policy_visit_keeps_its_seven_combinations(px):
    """tests/hostsim/host_light.hpp's visit serves today's seven combinations and returns false for every parallax variant and for the
    combinations it always refused."""
    L5 = levels_flag(5)
    seven = (0, AMBIENT_SH, L5, GLOSS | L5, GLOSS | L5 | AMBIENT_SH, GLOSS | L5 | ENV_BRDF, GLOSS | L5 | AMBIENT_SH | ENV_BRDF)
    assert [px.old_visit(f) for f in seven] == [1] * 7
    assert [px.old_visit(f | PARALLAX) for f in seven] == [0] * 7
    assert px.old_visit(L5 | AMBIENT_SH) == 0 and px.old_visit(ENV_BRDF) == 0


def test_host_body_refuses_what_the_entries_refuse(built_lib, px, gl):
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, _ = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, 2)
    q = dict(p, cube=with_probe(chain, dim, 2, probe_floats(*BOX)))
    rcs = [px.host_light_rc(c.pass_cb, q, flags, cube_dim=dim)
           for flags in (PARALLAX, PARALLAX | levels_flag(2), PARALLAX | GLOSS, PARALLAX | AMBIENT_SH, PARALLAX | GLOSS | levels_flag(1), box_flags(2))]
    assert rcs == [-1, -1, -1, -1, -1, 0]


# ---- without the flag --------------------------------------------------------------------------------------------------------------------

def test_flags_without_the_bit_give_the_frames_already_pinned(built_lib, px, eb, es, gl):
    """The harness without the flag goes through host_light itself: the gloss frame is the frozen gloss checker's and the split-sum
    frames are the split-sum checker's, whatever the probe volume's bytes hold."""
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    for levels in (2, 5):
        chain, dim = gloss_chain(gl, p, levels)
        q = with_view_normals(with_table_roughness(p, levels), eye_of(c.pass_cb))
        base = 1 | GLOSS | levels_flag(levels)
        want = gl.checker_light(pcb, dict(q, cube=chain), None, 3, 0.0, base, cube_dim=dim)
        for probe in (scene_probe(levels), np.full(12, np.nan, np.float32)):
            qq = dict(q, cube=with_probe(chain, dim, levels, probe, scene_block(es, p), eb.table()[0]))
            assert same_frame(px.host_light(c.pass_cb, qq, None, 3, 0.0, base, cube_dim=dim), want)
            for sh in (False, True):
                flags = base | ENV_BRDF | (AMBIENT_SH if sh else 0)
                assert same_frame(px.host_light(c.pass_cb, qq, None, 3, 0.0, flags, cube_dim=dim),
                                  eb.checker_light(pcb, qq, None, 3, 0.0, flags, cube_dim=dim)), (levels, sh)
