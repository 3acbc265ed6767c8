"""crychic_render_sky and crychic_sky_sun_colour on the CPU tier: the kernel body (csrc/sky_core.hpp, built for the host with the
workgroup and lane walk emulated) against the checker (tests/sky_ref, plain C from the definition in include/crychic_hip.h), byte for
byte on the whole corpus, behind guard bytes; what the corpus must reach, checked with the checker alone; face ranges; the refusals of
the real library, which need no device; and the sun colour's known answers."""
import ctypes as C
import math

import numpy as np
import pytest

import sky_host_lib as host
import sky_lib as sk


@pytest.fixture(scope="module")
def cases(built_lib):
    return sk.corpus()


def run_host(dim, params=None, face0=0, faces=6, misalign=0):
    """The kernel body into a guarded cube of 0xA5, `misalign` bytes past a 64-byte boundary; asserts the guard bytes."""
    raw, cube = sk.guarded((6, dim, dim, 4), misalign=misalign)
    groups = host.render_sky(cube, dim, params, face0, faces)
    assert groups == faces * ((dim + 31) // 32) * ((dim + 7) // 8)
    assert sk.guards_intact(raw, cube), "guard bytes changed"
    return cube


@pytest.mark.parametrize("dim", sk.DIMS)
def test_host_body_equals_checker(cases, dim):
    ran = 0
    for name, d, params in cases:
        if d != dim:
            continue
        ref, _ = sk.expected(name)
        got = run_host(dim, params, misalign=4 * (ran % 4))
        assert np.array_equal(got, ref), "%s: %d bytes differ" % (name, int((got != ref).sum()))
        assert (ref[..., 3] == 255).all()
        ran += 1
    assert ran >= 7


def test_the_corpus_reaches_what_it_must(cases):
    """With the checker alone: every size, sun, step count and altitude is there, and every branch the checker counts is taken."""
    assert {d for _, d, _ in cases} == set(sk.DIMS)
    for dim in sk.DIMS:
        mine = [p for _, d, p in cases if d == dim]
        assert {tuple(p["sunDir"]) for p in mine} >= set(sk.SUNS.values())
        assert {p.get("altitude") for p in mine} >= set(sk.ALTITUDES)
        assert {(p.get("viewSteps"), p.get("sunSteps")) for p in mine} >= set(sk.STEPS.values())
    total = dict.fromkeys(sk.COUNTERS, 0)
    for name, dim, params in cases:
        _, n = sk.expected(name)
        steps = dict(sk.DEFAULTS, **params)["viewSteps"]
        assert n["ground"] + n["sky"] == 6 * dim * dim and n["lit"] + n["blocked"] == 6 * dim * dim * steps, name
        assert n["sunlit_ground"] + n["dark_ground"] == n["ground"], name
        for k in total:
            total[k] += n[k]
    assert all(v > 0 for v in total.values()), total
    # the wide disc covers several texels; night is black all over; twilight has both lit and blocked samples in one cube
    for name in ("dim33_el30_wide_disc", "dim33_el5_wide_disc", "dim33_offaxis_wide_disc", "dim33_el30_wide_disc_alt50"):
        assert sk.expected(name)[1]["disc"] >= 4, name
    for name, dim, params in cases:
        _, n = sk.expected(name)
        if tuple(params["sunDir"]) == sk.SUNS["el-30"]:
            assert n["black"] == 6 * dim * dim and n["lit"] == 0, name
        if tuple(params["sunDir"]) == sk.SUNS["el-3"] and dim >= 8:
            assert n["lit"] > 0 and n["blocked"] > 0 and n["black"] < 6 * dim * dim, name


@pytest.mark.parametrize("name", ["dim8_el5_sdef_alt50", "dim33_el30_wide_disc", "dim3_offaxis_sdef_alt0"])
def test_face_ranges_stitch_to_the_whole_cube(cases, name):
    """Every split of the six faces into two calls: each call equals the checker's, writes nothing outside its faces, and the two
    stitch to the whole."""
    _, dim, params = {c[0]: c for c in cases}[name]
    whole, _ = sk.expected(name)
    for k in range(7):
        stitched = np.full(whole.shape, sk.GUARD, np.uint8)
        for face0, faces in ((0, k), (k, 6 - k)):
            got = run_host(dim, params, face0, faces)
            ref, _ = sk.checker(dim, params, face0, faces)
            assert np.array_equal(got, ref), (name, face0, faces)
            assert (got[:face0] == sk.GUARD).all() and (got[face0 + faces:] == sk.GUARD).all(), "a face outside the range was written"
            stitched[face0:face0 + faces] = got[face0:face0 + faces]
        assert np.array_equal(stitched, whole), (name, k)
    # one face at a time, in place on one cube
    cube = np.full(whole.shape, sk.GUARD, np.uint8)
    for f in (3, 0, 5, 1, 4, 2):
        host.render_sky(cube, dim, params, f, 1)
    assert np.array_equal(cube, whole)


def test_default_params(built_lib):
    p = built_lib.SkyParams()
    assert C.sizeof(p) == 48 and built_lib.lib.crychic_sky_default_params(C.byref(p)) == 0
    d = sk.DEFAULTS
    assert tuple(p.sunDir) == tuple(np.float32(d["sunDir"])) and tuple(p.reserved) == (0, 0)
    for k in ("altitude", "sunIntensity", "exposure", "sunAngularRadius", "groundAlbedo"):
        assert getattr(p, k) == np.float32(d[k]), k
    assert (p.viewSteps, p.sunSteps) == (d["viewSteps"], d["sunSteps"])
    assert bytes(p) == sk.params_array().tobytes()
    assert built_lib.lib.crychic_sky_default_params(None) == -1
    assert (built_lib.SKY_MAX_VIEW_STEPS, built_lib.SKY_MAX_SUN_STEPS) == (64, 32)
    q = built_lib.SkyParams.default(sunDir=(1, 2, 3), viewSteps=3, exposure=0.5)
    assert (tuple(q.sunDir), q.viewSteps, q.exposure, q.sunSteps) == ((1.0, 2.0, 3.0), 3, 0.5, d["sunSteps"])


def refusal_cases(P):
    """[(keyword arguments of a call, a word of the message)]: every refusal include/crychic_hip.h lists."""
    def prm(**kw):
        return P.default(**kw)
    bad_res = prm()
    bad_res.reserved[1] = 1
    out = [(dict(cube=None), "null argument"), (dict(cube=0x10000002), "aligned"), (dict(cube=0x10000001), "aligned"),
           (dict(dim=0), "face size"), (dict(dim=1), "face size"), (dict(dim=8193), "face size"), (dict(dim=0xFFFFFFFF), "face size"),
           (dict(face0=7, faces=0), "six faces"), (dict(face0=0, faces=7), "six faces"), (dict(face0=4, faces=3), "six faces"),
           (dict(face0=6, faces=1), "six faces"), (dict(face0=0xFFFFFFFF, faces=2), "six faces"), (dict(face0=2, faces=0xFFFFFFFF), "six faces"),
           (dict(params=prm(sunDir=(0, 0, 0))), "zero vector"), (dict(params=prm(sunDir=(-0.0, 0.0, -0.0))), "zero vector"),
           (dict(params=bad_res), "reserved")]
    for c in range(3):
        for bad in (math.nan, math.inf, -math.inf):
            v = [0.1, 0.2, 0.3]
            v[c] = bad
            out.append((dict(params=prm(sunDir=v)), "sunDir"))
    for field, lo, hi in (("altitude", 0.0, 50.0), ("sunIntensity", 0.0, 65536.0), ("exposure", 0.0, 65536.0), ("sunAngularRadius", 0.0, 0.5),
                          ("groundAlbedo", 0.0, 1.0)):
        for bad in (math.nan, math.inf, -math.inf, float(np.nextafter(np.float32(lo), np.float32(-1))), float(np.nextafter(np.float32(hi), np.float32(1e9)))):
            out.append((dict(params=prm(**{field: bad})), field))
    for field, hi in (("viewSteps", 64), ("sunSteps", 32)):
        for bad in (0, hi + 1, 0xFFFFFFFF):
            out.append((dict(params=prm(**{field: bad})), field))
    return out


def accepted_cases(P):
    """Keyword arguments at the edges of what is valid."""
    return [dict(), dict(dim=2), dict(dim=8192), dict(face0=6, faces=0), dict(face0=0, faces=0), dict(face0=5, faces=1), dict(params=None),
            dict(params=P.default(altitude=0.0, sunIntensity=0.0, exposure=0.0, sunAngularRadius=0.0, groundAlbedo=0.0, viewSteps=1, sunSteps=1)),
            dict(params=P.default(altitude=50.0, sunIntensity=65536.0, exposure=65536.0, sunAngularRadius=0.5, groundAlbedo=1.0, viewSteps=64, sunSteps=32)),
            dict(params=P.default(sunDir=(0.0, -1e-30, 0.0))), dict(params=P.default(sunDir=(3e38, -3e38, 3e38)))]


def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, P = built_lib.lib, built_lib.SkyParams

    def call(cube=0x10000000, dim=64, face0=0, faces=6, params=P.default()):        # the address is never dereferenced
        rc = lib.crychic_render_sky(None, cube, dim, face0, faces, None if params is None else C.byref(params), None)
        return rc, lib.crychic_last_error().decode()
    for kw in accepted_cases(P):
        assert call(**kw) == (-1, "null context"), kw
    for kw, word in refusal_cases(P):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    # the sun colour refuses the same parameters
    rgb = (C.c_float * 3)(7.0, 7.0, 7.0)
    for kw, word in refusal_cases(P):
        if "params" in kw:
            assert lib.crychic_sky_sun_colour(C.byref(kw["params"]), rgb) == -1 and word in lib.crychic_last_error().decode(), kw
            assert tuple(rgb) == (7.0, 7.0, 7.0), "a refusal wrote the colour"
    assert lib.crychic_sky_sun_colour(None, None) == -1 and "null argument" in lib.crychic_last_error().decode()
    assert lib.crychic_sky_sun_colour(None, rgb) == 0 and tuple(rgb) == tuple(sk.sun_colour())


def lib_sun_colour(built_lib, params):
    rgb = (C.c_float * 3)()
    p = built_lib.SkyParams.from_buffer_copy(sk.params_array(params).tobytes())
    assert built_lib.lib.crychic_sky_sun_colour(C.byref(p), rgb) == 0
    return np.array(rgb, np.float32)


def test_sun_colour_is_the_checkers_bit_for_bit(cases, built_lib):
    """The library's host code, the host build of the body and the checker, on every parameter set of the corpus."""
    seen = set()
    for _, _, params in cases:
        key = repr(sorted(params.items()))
        if key in seen:
            continue
        seen.add(key)
        want = sk.sun_colour(params).view(np.uint32)
        assert np.array_equal(host.sun_colour(params).view(np.uint32), want), params
        assert np.array_equal(lib_sun_colour(built_lib, params).view(np.uint32), want), params
    assert len(seen) >= 20


# the largest relative error of a channel of the sun colour at the default sunSteps = 8 against the closed form, as measured by
# tests/sky_quality.py and recorded in profiles/sky_quality.txt: the quadrature error of the sun march (and the 60 km shell, which
# cuts 5.5e-4 of the Rayleigh column).  The assertion is at twice that.
ZENITH_QUADRATURE_ERROR = 4.629e-3


def test_sun_colour_known_answers(built_lib):
    d = sk.DEFAULTS
    beta_r, beta_m = np.array([5.8e-3, 13.5e-3, 33.1e-3]), 21e-3
    want = d["sunIntensity"] * np.exp(-(beta_r * 8.0 + 1.1 * beta_m * 1.2))
    zenith = dict(sunDir=(0.0, 1.0, 0.0), altitude=0.0)
    errs = {}
    for n in (4, 8, 16, 32):
        got = lib_sun_colour(built_lib, dict(zenith, sunSteps=n)).astype(np.float64)
        errs[n] = float(np.max(np.abs(got - want) / want))
    print("zenith sun colour, relative error by sunSteps:", errs)
    assert d["sunSteps"] == 8 and errs[8] <= 2.0 * ZENITH_QUADRATURE_ERROR, errs
    assert errs[4] > errs[8] > errs[16] > errs[32], "halving the step does not shrink the error"
    # the planet hides a sun 30 degrees below the horizon: exactly zero, at either altitude
    for alt in sk.ALTITUDES + (d["altitude"],):
        assert lib_sun_colour(built_lib, dict(sunDir=sk.sun_at(-30), altitude=alt)).tolist() == [0.0, 0.0, 0.0]
    # a lower sun is redder and dimmer
    hi, lo = lib_sun_colour(built_lib, dict(sunDir=sk.sun_at(60))), lib_sun_colour(built_lib, dict(sunDir=sk.sun_at(3)))
    assert (lo < hi).all() and lo[0] > lo[1] > lo[2] and lo[2] / lo[0] < hi[2] / hi[0]
    # sunDir is normalised by the definition
    assert np.array_equal(lib_sun_colour(built_lib, dict(sunDir=(0.0, 2.0, 0.0))), lib_sun_colour(built_lib, dict(sunDir=(0.0, 0.25, 0.0))))
