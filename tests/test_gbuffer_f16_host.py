"""G-buffer plane formats (include/crychic_hip.h CRYCHIC_GBUFFER_G*_F16), CPU tier.  The format is storage
only, so the whole contract is two statements against code that is frozen:
  1. light(planes in any format mix) == checker light(those planes widened to fp32), RGBA8 and radiance bits;
  2. producer(format mix) == float_to_half(oracle rasteriser's fp32 planes) on the half planes; everything else unchanged.
Here the product's bodies run on the host (tests/hostsim: hs_light, hs_rasterize); tests/test_gbuffer_f16_gpu.py repeats the
statements on the device."""
import ctypes as C

import numpy as np
import pytest

import fuzz_util
import gbuffer_f16_lib as gf
import hostsim_lib
import oracle_lib
import point_shadow_lib
import raster_util
import scene_util
from local_lights_util import FIX_ALL, _cpu, random_maps, spot_transforms, spots_for_test, transposed, with_transforms


def known_answer_floats():
    """(float32 values, expected binary16 bits): ties to even, the largest finite value and the overflow threshold, subnormals, +-0."""
    f = np.float32
    cases = [
        (f(0.0), 0x0000), (f(-0.0), 0x8000), (f(1.0), 0x3C00), (f(-2.0), 0xC000),
        (f(1.0) + f(2.0 ** -11), 0x3C00),                # tie between 1 and 1 + 2^-10: to even (down)
        (f(1.0) + f(3 * 2.0 ** -11), 0x3C02),            # tie between 1 + 2^-10 and 1 + 2^-9: to even (up)
        (f(1.0) + f(2.0 ** -11) + f(2.0 ** -23), 0x3C01),  # just above the tie: up
        (f(65504.0), 0x7BFF),                            # the largest finite half
        (f(65519.996), 0x7BFF),                          # below the overflow threshold 65520: rounds down to it
        (f(65520.0), 0x7C00), (f(-65520.0), 0xFC00),     # the tie at the top goes to even = infinity
        (f(1.0e30), 0x7C00), (f(np.inf), 0x7C00), (f(-np.inf), 0xFC00),
        (f(2.0 ** -24), 0x0001), (f(-2.0 ** -24), 0x8001),   # the smallest subnormal
        (f(2.0 ** -25), 0x0000),                         # tie between 0 and the smallest subnormal: to even (0)
        (f(2.0 ** -25) + f(2.0 ** -40), 0x0001),         # just above it
        (f(3 * 2.0 ** -25), 0x0002),                     # tie between subnormals 1 and 2: to even (2)
        (f(2.0 ** -14), 0x0400), (f(2.0 ** -14) - f(2.0 ** -24), 0x03FF),   # the smallest normal, the largest subnormal
        (f(1.0e-10), 0x0000), (f(-1.0e-10), 0x8000),
    ]
    return np.array([c[0] for c in cases], np.float32), np.array([c[1] for c in cases], np.uint16)


def test_float_to_half_known_answers(built_lib):
    """raster_core.hpp float_to_half on the host: the hand-derived answers, numpy's conversion on them and on 20000 random floats
    around every interesting range; half_to_float is exact (numpy's widening) for all 65536 encodings, NaNs as NaNs."""
    lib = hostsim_lib.load()
    x, want = known_answer_floats()
    got = lib.float_to_half(x)
    assert got.tolist() == want.tolist(), [(float(a), hex(b), hex(c)) for a, b, c in zip(x, got, want) if b != c]
    with np.errstate(over="ignore"):
        assert x.astype(np.float16).view(np.uint16).tolist() == want.tolist()
    rng = np.random.default_rng(1)
    r = np.concatenate([rng.standard_normal(5000) * s for s in (1.0, 1e-6, 3e4, 1e-4)]).astype(np.float32)
    with np.errstate(over="ignore"):
        assert np.array_equal(lib.float_to_half(r), r.astype(np.float16).view(np.uint16))
    h = np.arange(65536, dtype=np.uint16)
    wide = lib.half_to_float(h)
    ref = h.view(np.float16).astype(np.float32)
    assert fuzz_util.same_floats(wide, ref)
    assert np.isnan(wide).sum() == 2 * 1023 and np.array_equal(wide[1:1024], (np.arange(1, 1024) * 2.0 ** -24).astype(np.float32))


def test_torch_conversion_is_float_to_half(built_lib):
    """Crychic.load_scene converts incoming fp32 planes with torch.Tensor.to(torch.float16): the same rounding as float_to_half."""
    import torch
    x, want = known_answer_floats()
    rng = np.random.default_rng(2)
    r = np.concatenate([x] + [(rng.standard_normal(4000) * s).astype(np.float32) for s in (1.0, 1e-6, 3e4, 1e-4)])
    got = torch.from_numpy(r).to(torch.float16).numpy().view(np.uint16)
    assert np.array_equal(got, hostsim_lib.load().float_to_half(r))
    assert got[:len(want)].tolist() == want.tolist()


def test_plane_bytes_and_stray_producer_flags(built_lib):
    lib = built_lib.lib
    for W, H in ((3840, 2160), (322, 190)):
        for flags in gf.MIXES:
            for plane in range(3):
                want = W * H * (8 if flags & (gf.G0_F16 << plane) else 16)
                assert lib.crychic_gbuffer_plane_bytes(W, H, flags | 0x701, plane) == want        # other bits of the word do not count
        assert lib.crychic_gbuffer_plane_bytes(W, H, 0, 3) == 0 and lib.crychic_gbuffer_plane_bytes(W, H, 0, -1) == 0
    assert sum(lib.crychic_gbuffer_plane_bytes(3840, 2160, gf.MIXED, k) for k in range(3)) == 3840 * 2160 * 32
    assert sum(lib.crychic_gbuffer_plane_bytes(3840, 2160, gf.ALL_F16, k) for k in range(3)) == 3840 * 2160 * 24
    assert (built_lib.lib.crychic_gbuffer_plane_bytes.restype, gf.F16_MASK) == (C.c_size_t, 0x7000)
    # bits outside the three are refused before anything else is looked at (no device needed)
    for stray in (0x1, 0x100, 0x800, 0x8000, 0x10000, 0x80000000, gf.ALL_F16 | 0x8000):
        rc = lib.crychic_draw_gbuffer_formats(None, None, None, 0, None, 0, None, 0, None, None, None, None, stray, None, 64, 64, 0, 0,
                                              None, 0, None)
        assert rc == -1 and b"gbufferFlags" in lib.crychic_last_error(), hex(stray)
    rc = lib.crychic_draw_gbuffer_formats(None, None, None, 0, None, 0, None, 0, None, None, None, None, gf.ALL_F16, None, 64, 64, 0, 0,
                                          None, 0, None)
    assert rc == -1 and b"gbufferFlags" not in lib.crychic_last_error()         # valid flags: the next check (null targets) speaks


# ---- statement 1: lighting -------------------------------------------------------------------------------------------------------

def _special_texels(p, seed):
    """Texels that overflow fp16 (|x| > 65504 -> inf), fp16 subnormals and values that round to them, in covered pixels of every plane."""
    rng = np.random.default_rng(seed)
    q = {k: (v.copy() if k in ("g0", "g1", "g2") else v) for k, v in p.items()}
    H, W = p["depth"].shape
    ys, xs = np.nonzero((p["depth"] & 0xFFFFFF) < 0xFFFFFF)
    pick = rng.choice(len(ys), size=min(len(ys), 240), replace=False)
    vals = np.array([7.0e4, -1.0e5, 65520.0, 65519.0, 3.0e38, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -15, 5.0e-8, 2.0 ** -25, 1.0e-9],
                    np.float32)
    for n, i in enumerate(pick):
        plane = q["g%d" % (n % 3)]
        plane[ys[i], xs[i], (n // 3) % 4] = vals[(n // 12) % len(vals)]
    return q


def _local_case(W, H):
    """The reference scene with points + spots + shadowed spots + shadowed points (test_point_shadows' frame set-up)."""
    from test_point_shadows import point_transforms, random_cubes, shadowed_points
    _, p, c, _ = _cpu(W, H)
    spots, points = spots_for_test(), shadowed_points()
    cb, pcb = with_transforms(c.pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 8)])
    maps = random_maps(3, 48, 2)
    cubes = random_cubes(4, 48, 9)
    projs = [sp.reshape(-1) for _, _, sp in point_transforms(points, 4, 48)]
    return p, cb, pcb, dict(points=points, spots=spots, maps=maps, cubes=cubes, projs=projs)


def _same(got, ref):
    return np.array_equal(got[0], ref[0]) and fuzz_util.same_floats(got[1], ref[1])


@pytest.mark.parametrize("local", [False, True], ids=["no_local_lights", "local_lights"])
@pytest.mark.parametrize("chain", [False, True], ids=["level0", "chain"])
def test_host_body_matches_checker_on_widened_planes(built_lib, oracle, local, chain):
    """All eight format mixes x radius 0 / 2.5 / dim x Q fixes off / on x sky on / off x cube chain off / on x {no local lights;
    points + spots + shadowed spots + shadowed points}: the host body on the packed planes == the checker on the widened planes,
    RGBA8 and radiance bits.  The checker is the oracle without local lights, point_shadow_lib's with them.  The planes are the
    reference scene's with texels that overflow fp16 and fp16 subnormals added."""
    from crychic_renderer_amd import geometry as g
    W, H = 98, 66
    p, cb, pcb, lights = _local_case(W, H)
    if not local:
        lights = {}
    p = _special_texels(p, 5)
    kw, levels = {}, 0
    if chain:
        cube, levels = g.cube_mip_chain(p["cube"])
        p = dict(p, cube=cube)
        kw = dict(cube_dim=32)
    rng = np.random.default_rng(3)
    ao = rng.integers(20000, 65535, (H // 2, W // 2), dtype=np.uint16)
    lib, ps = hostsim_lib.load(), point_shadow_lib.load()
    changed = 0
    for mix in gf.MIXES:
        packed = gf.pack_planes(p, mix)
        wide = gf.widen_planes(packed)
        assert gf.mix_of(packed) == mix
        for radius in (0.0, 2.5 / 256):
            for fixes, ndl, ambient in ((0, 1, None), (FIX_ALL, 3, ao)):
                for sky in (1, 0):
                    flags = fixes | sky | ((levels & 15) << 16)
                    got = lib.light_frame(cb, packed, ambient, ndl, radius, flags, **lights, **kw)
                    if local:
                        ref = ps.checker(pcb, wide, ambient, ndl, radius, flags, **lights, **kw)
                    else:
                        ref = oracle.deferred_light(pcb, wide["g0"], wide["g1"], wide["g2"], wide["depth"], ambient, wide["shadow"], wide["cube"],
                                                    ndl, radius, sky=bool(sky), want_radiance=True, fixes=fixes, cube_levels=levels, **kw)
                    assert _same(got, ref), (hex(mix), radius, fixes, sky)
        if mix:         # the format is not a no-op: the packed planes light differently from the fp32 ones
            full = lib.light_frame(cb, p, None, 1, 0.0, 1 | ((levels & 15) << 16), **lights, **kw)
            changed += not np.array_equal(full[1].view(np.uint32), got[1].view(np.uint32))
    assert changed == 7


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_host_body_special_value_planes(built_lib, oracle, seed):
    """fuzz_util's planes (inf, NaN, zero-length normals, 1e30 positions: NaN and inf survive the conversion, 1e30 overflows to inf)
    in every format mix, any NaN equal to any NaN: the oracle without local lights, point_shadow_lib's checker with point and spot
    lights."""
    from local_lights_util import points_for_test
    W, H, planes, c, knobs = fuzz_util.random_case(100 + seed, built_lib, size=(66, 50))
    p = {k: planes[k] for k in ("g0", "g1", "g2", "depth", "shadow", "cube")}
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    lib, ps = hostsim_lib.load(), point_shadow_lib.load()
    points, spots = points_for_test(), spots_for_test()
    fixes = FIX_ALL if seed & 1 else 0
    for mix in gf.MIXES:
        packed = gf.pack_planes(p, mix)
        wide = gf.widen_planes(packed)
        flags = fixes | knobs["sky"]
        got = lib.light_frame(c.pass_cb, packed, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags)
        ref = oracle.deferred_light(pcb, wide["g0"], wide["g1"], wide["g2"], wide["depth"], None, wide["shadow"], wide["cube"],
                                    knobs["numDirLights"], knobs["pcfSearchRadius"], sky=bool(knobs["sky"]), want_radiance=True, fixes=fixes)
        assert _same(got, ref), (seed, hex(mix))
        got = lib.light_frame(c.pass_cb, packed, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, points=points, spots=spots)
        ref = ps.checker(pcb, wide, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, points=points, spots=spots)
        assert _same(got, ref), (seed, hex(mix), "local")


def test_host_body_row_range(built_lib, oracle):
    """A row range of a mixed frame == the same rows of the whole frame; rows outside are not written."""
    W, H = 98, 66
    p, cb, pcb, lights = _local_case(W, H)
    packed = gf.pack_planes(p, gf.MIXED)
    lib = hostsim_lib.load()
    whole = lib.light_frame(cb, packed, None, 3, 0.0, 1, **lights)
    part = lib.light_frame(cb, packed, None, 3, 0.0, 1, row0=20, rows=30, **lights)
    assert np.array_equal(part[0][20:50], whole[0][20:50]) and not part[0][:20].any() and not part[0][50:].any()


# ---- statement 2: producers ------------------------------------------------------------------------------------------------------

def _scene(name, tmp_path, oracle):
    from crychic_renderer_amd import geometry as g
    if name == "reference":
        W, H = 160, 90
        cs = scene_util.cpu_scene(W, H, 128, 16)["consts"]
        return W, H, cs, g.cascade_scene_items(), g.reference_materials(), g.procedural_textures(32)
    W, H = 128, 128
    cs = raster_util.frame_constants(W, H, 128)
    v, idx = oracle_lib.load_mesh_text(oracle, raster_util.mesh_text("skull", tmp_path))
    return W, H, cs, raster_util.c1_items(v, idx), g.reference_materials(), None


@pytest.mark.parametrize("name", ["reference", "skull"])
def test_resolve_matches_float_to_half_of_oracle_planes(built_lib, oracle, tmp_path, name):
    """The format-aware resolve on the host, every mix, G-buffer pass alone and fused: a half plane == numpy.float16 of
    oracle_lib.rasterize's fp32 plane bit for bit (cleared texels: zero bits), float planes, depth and the normal map are the
    oracle's; a row range writes the rows and nothing else."""
    W, H, cs, items, mats, tex = _scene(name, tmp_path, oracle)
    view = np.array(cs.pass_cb.View, np.float32); vp = np.array(cs.pass_cb.ViewProj, np.float32)
    omats = mats.view(oracle_lib.MATERIAL_DT)
    gb = oracle_lib.rasterize(oracle, 2, view, vp, items, omats, tex, W, H)
    nd = oracle_lib.rasterize(oracle, 1, view, vp, items, omats, tex, W, H)
    clear = (gb["depth"] & 0xFFFFFF) == 0xFFFFFF
    assert 0.02 < clear.mean() < 0.98
    lib = hostsim_lib.load()
    mixes = gf.MIXES if name == "reference" else [gf.MIXED, gf.ALL_F16]
    for mix in mixes:
        for fused in (False, True):
            r = lib.rasterize(3 if fused else 2, view, vp, items, mats, tex, W, H, mix=mix)
            assert np.array_equal(r["depth"], gb["depth"])
            if fused:
                assert np.array_equal(r["normal"].view(np.uint16), nd["normal"].view(np.uint16))
            for k in range(3):
                ref = gb["g%d" % k]
                if mix & (gf.G0_F16 << k):
                    assert r["g%d" % k].dtype == np.float16
                    assert np.array_equal(r["g%d" % k].view(np.uint16), ref.astype(np.float16).view(np.uint16)), (hex(mix), k)
                    assert not r["g%d" % k].view(np.uint16)[clear].any()
                else:
                    assert np.array_equal(r["g%d" % k].view(np.uint32), ref.view(np.uint32)), (hex(mix), k)
    # rows [r0, r0 + rn): the G-buffer inside, the fill byte outside; the pass alone limits depth too, the fused pass does not
    r0, rn = 22, 40
    for fused in (False, True):
        r = lib.rasterize(3 if fused else 2, view, vp, items, mats, tex, W, H, mix=gf.MIXED, g_row0=r0, g_rows=rn, fill=0xCD)
        for k in range(3):
            want = gb["g%d" % k] if k == 0 else gb["g%d" % k].astype(np.float16)
            raw, wraw = r["g%d" % k].view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
            assert np.array_equal(raw[r0:r0 + rn], wraw[r0:r0 + rn])
            assert (raw[:r0] == 0xCD).all() and (raw[r0 + rn:] == 0xCD).all()
        assert np.array_equal(r["depth"][r0:r0 + rn], gb["depth"][r0:r0 + rn])
        if fused:
            assert np.array_equal(r["depth"], gb["depth"]) and np.array_equal(r["normal"].view(np.uint16), nd["normal"].view(np.uint16))
        else:
            assert (r["depth"][:r0] == 0xCDCDCDCD).all() and (r["depth"][r0 + rn:] == 0xCDCDCDCD).all()
