"""G-buffer plane formats (include/crychic_hip.h CRYCHIC_GBUFFER_G*_F16) on the device.  The two statements of
tests/test_gbuffer_f16_host.py, now for the kernels: every lighting entry on planes in any format mix == the frozen checker on those
planes widened to fp32, and the format-aware producer == the host harness (itself == numpy.float16 of the oracle rasteriser's planes),
bit for bit; then the whole path through Crychic, a hipGraph, a 4K frame and the C++ veneer."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fuzz_util
import gbuffer_f16_lib as gf
import hostsim_lib
import oracle_lib
import point_shadow_lib
import raster_util
import scene_util
from local_lights_util import (FIX_ALL, _app, _dev_lights, _device_scene, random_maps, spot_transforms, spots_for_test, transposed,
                               with_transforms)

pytestmark = pytest.mark.gpu


def _to_dev(ctx, a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(ctx.device)


def _packed_dev(ctx, p, dev, mix):
    """(numpy planes in the formats of mix, the same on the device, the widened numpy planes the checkers get)."""
    packed = gf.pack_planes(p, mix)
    d = dict(dev)
    for k in ("g0", "g1", "g2"):
        d[k] = _to_dev(ctx, packed[k])
    return packed, d, gf.widen_planes(packed)


def _spot_desc(dev_maps):
    from crychic_renderer_amd._lib import SpotShadows
    d = SpotShadows()
    d.count, d.dim = dev_maps.shape[0], dev_maps.shape[1]
    for k in range(dev_maps.shape[0]):
        d.maps[k] = dev_maps[k].data_ptr()
    return d


def _point_desc(dev_cubes, projs):
    from crychic_renderer_amd._lib import PointShadows
    d = PointShadows()
    d.count, d.dim = dev_cubes.shape[0], dev_cubes.shape[2]
    for k in range(dev_cubes.shape[0]):
        d.maps[k] = dev_cubes[k].data_ptr()
        d.shadowProj[k][:] = [float(v) for v in np.asarray(projs[k], np.float32).reshape(-1)]
    return d


ENTRIES = ("light", "points", "spots", "spots_shadowed", "point_shadows")


def _light(lib, ctx, entry, cb, dev, W, H, flags, dp=(None, 0), ds=(None, 0), sdesc=None, pdesc=None, ndl=3, radius=0.0, ambient=None,
           row0=0, rows=None, out=None, rad=None, cube=None, cube_dim=32, shadow_dim=256):
    """One crychic_deferred_light* call; `flags` carries the planes' CRYCHIC_GBUFFER_* bits (taken from the device tensors' dtypes)."""
    import torch
    from crychic_renderer_amd import gbuffer_flags
    from crychic_renderer_amd.renderer import _ptr, _stream
    rows = H - row0 if rows is None else rows
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device) if out is None else out
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device) if rad is None else rad
    sh = (C.c_void_p * 4)(*[dev["shadow"][k].data_ptr() for k in range(4)])
    flags = int(flags) | gbuffer_flags([dev["g0"], dev["g1"], dev["g2"]])
    args = [ctx.handle, C.byref(cb), _ptr(dev["g0"]), _ptr(dev["g1"]), _ptr(dev["g2"]), _ptr(dev["depth"]), _ptr(ambient), sh, shadow_dim,
            _ptr(cube if cube is not None else dev["cube"]), cube_dim, _ptr(out), _ptr(rad), W, H, row0, rows, ndl, radius, flags]
    points, spots = [_ptr(dp[0]), dp[1]], [_ptr(ds[0]), ds[1]]
    sd, pd = (None if sdesc is None else C.byref(sdesc)), (None if pdesc is None else C.byref(pdesc))
    st = _stream(ctx.device)
    if entry == "light":
        rc = lib.crychic_deferred_light(*args, st)
    elif entry == "points":
        rc = lib.crychic_deferred_light_points(*args, *points, st)
    elif entry == "spots":
        rc = lib.crychic_deferred_light_spots(*args, *points, *spots, st)
    elif entry == "spots_shadowed":
        rc = lib.crychic_deferred_light_spots_shadowed(*args, *points, *spots, sd, st)
    else:
        rc = lib.crychic_deferred_light_point_shadows(*args, *points, *spots, sd, pd, st)
    return rc, out, rad


class _Lights:
    """The local lights of the tests: points + spots + 3 shadowed spots + 4 shadowed points, on the device and for the checker."""

    def __init__(self, ctx, pass_cb, map_dim=64, cube_dim=48):
        from test_point_shadows import point_transforms, random_cubes, shadowed_points
        self.points, self.spots = shadowed_points(), spots_for_test()
        self.cb, self.pcb = with_transforms(pass_cb, [transposed(st) for _, _, st in spot_transforms(self.spots, 8)])
        self.maps = random_maps(3, map_dim, 5)
        self.cubes = random_cubes(4, cube_dim, 8)
        self.projs = [sp.reshape(-1) for _, _, sp in point_transforms(self.points, 4, cube_dim)]
        self.dp, self.ds = _dev_lights(ctx, self.points), _dev_lights(ctx, self.spots)
        self.mdev, self.cdev = _to_dev(ctx, self.maps), _to_dev(ctx, self.cubes)
        self.sdesc, self.pdesc = _spot_desc(self.mdev), _point_desc(self.cdev, self.projs)

    def of(self, entry):
        """(device arguments of _light, checker arguments) for what `entry` takes."""
        dev, chk = {}, {}
        if entry != "light":
            dev["dp"] = self.dp; chk["points"] = self.points
        if entry in ("spots", "spots_shadowed", "point_shadows"):
            dev["ds"] = self.ds; chk["spots"] = self.spots
        if entry in ("spots_shadowed", "point_shadows"):
            dev["sdesc"] = self.sdesc; chk["maps"] = self.maps
        if entry == "point_shadows":
            dev["pdesc"] = self.pdesc; chk["cubes"] = self.cubes; chk["projs"] = self.projs
        return dev, chk


def _checker(oracle, entry, pcb, wide, ambient, ndl, radius, flags, chk, **kw):
    """The frozen checker on the widened planes: the oracle where it covers the case (no local lights), point_shadow_lib's otherwise."""
    if entry == "light":
        return oracle.deferred_light(pcb, wide["g0"], wide["g1"], wide["g2"], wide["depth"], ambient, wide["shadow"], wide["cube"], ndl, radius,
                                     sky=bool(flags & 1), want_radiance=True, fixes=flags & FIX_ALL, cube_levels=(flags >> 16) & 15,
                                     cube_dim=kw.get("cube_dim"))
    return point_shadow_lib.load().checker(pcb, wide, ambient, ndl, radius, flags, **chk, **kw)


def _assert_same(out, rad, ref, what):
    assert np.array_equal(out.cpu().numpy(), ref[0]), what
    assert fuzz_util.same_floats(rad.cpu().numpy(), ref[1]), what


# ---- the conversions themselves, through one producer / lighting round trip ------------------------------------------------------

def test_known_answers_round_trip_on_device(built_lib, oracle):
    """float_to_half and half_to_float on the device (subnormals included: gfx950 has to keep them in both conversions).  The
    known-answer values go in as material constants -- GeometryPass writes DiffuseAlbedo * 1, Roughness and Metalness through
    unchanged -- so the half planes the producer writes must hold exactly the expected bits; the lighting pass then reads them with an
    ambient light of 2^20 and no other light, which brings a subnormal albedo (2^-24 .. 2^-15) up to a visible radiance that a
    flushed conversion would lose, and must equal the oracle on the widened planes."""
    import torch
    from test_gbuffer_f16_host import known_answer_floats
    from crychic_renderer_amd import Context, SceneGeometry, geometry as g, scene
    from crychic_renderer_amd._lib import PassConstants
    W = H = 4
    ctx = Context(0)
    x, want = known_answer_floats()
    x = np.concatenate([x, np.zeros((-len(x)) % 5, np.float32)]); want = np.concatenate([want, np.zeros(len(x) - len(want), np.uint16)])
    consts = scene.Constants(W, H, 16)
    grid = g.create_grid(20.0, 30.0, 60, 40)
    items = [(grid[0], grid[1], g.make_instances([g.world_matrix()], [0]))]
    cb = PassConstants.from_buffer_copy(consts.pass_cb)
    cb.AmbientLight[:] = [2.0 ** 20] * 4
    pcb = oracle_lib.as_oracle_cb(cb, oracle_lib.OrPassConstants)
    shadow = torch.full((4, 16, 16), 0xFFFFFF, dtype=torch.int32, device=ctx.device)
    cube = torch.zeros((6, 2, 2, 4), dtype=torch.uint8, device=ctx.device)
    lib = hostsim_lib.load()
    seen_subnormal_light = 0
    for i in range(0, len(x), 5):
        v, w = x[i:i + 5], want[i:i + 5]
        mats = g.reference_materials()[:1].copy()
        mats[0]["DiffuseAlbedo"] = (v[0], v[1], v[2], 1.0); mats[0]["Roughness"] = v[3]; mats[0]["Metalness"] = v[4]
        mats[0]["DiffuseMapIndex"] = mats[0]["NormalMapIndex"] = 99           # no texture bound: the sampler's white / flat normal
        geo = SceneGeometry(ctx, items, mats, None)
        gb = [torch.full((H, W, 4), -1, dtype=torch.float16, device=ctx.device) for _ in range(3)]
        depth = torch.zeros((H, W), dtype=torch.int32, device=ctx.device)
        geo.DrawGBuffer(cb, gb, depth)
        torch.cuda.synchronize()
        d = depth.cpu().numpy().view(np.uint32)
        cov = (d & 0xFFFFFF) < 0xFFFFFF
        assert cov[H - 1].all() and not cov[0].any()                          # ground at the bottom, sky (the clear value) at the top
        g0, g1, g2 = (t.cpu().numpy() for t in gb)
        bits0, bits1 = g0.view(np.uint16), g1.view(np.uint16)
        assert (bits1[cov][:, :3] == w[:3]).all() and (bits1[cov][:, 3] == w[3]).all() and (bits0[cov][:, 3] == w[4]).all(), (v, w)
        assert not bits0[~cov].any() and not bits1[~cov].any() and not g2.view(np.uint16)[~cov].any()
        host = lib.rasterize(2, np.array(cb.View, np.float32), np.array(cb.ViewProj, np.float32), items, mats, None, W, H, mix=gf.ALL_F16)
        for k, t in enumerate((g0, g1, g2)):
            assert np.array_equal(t.view(np.uint16), host["g%d" % k].view(np.uint16)), k
        dev = {"g0": gb[0], "g1": gb[1], "g2": gb[2], "depth": depth, "shadow": shadow, "cube": cube}
        rc, out, rad = _light(built_lib.lib, ctx, "light", cb, dev, W, H, 0, ndl=0, cube_dim=2, shadow_dim=16)
        built_lib.check(rc)
        torch.cuda.synchronize()
        wide = {"g0": g0.astype(np.float32), "g1": g1.astype(np.float32), "g2": g2.astype(np.float32), "depth": d,
                "shadow": shadow.cpu().numpy().view(np.uint32), "cube": cube.cpu().numpy()}
        ref = _checker(oracle, "light", pcb, wide, None, 0, 0.0, 0, {})
        _assert_same(out, rad, ref, (v, w))
        r = rad.cpu().numpy()[cov]
        sub = [c for c in range(3) if 0 < (w[c] & 0x7FFF) < 0x0400]
        for c in sub:
            assert (r[:, c] != 0).all(), (v, c)                              # the subnormal albedo reached the arithmetic
        seen_subnormal_light += len(sub)
    assert seen_subnormal_light >= 3
    ctx.close()


# ---- statement 1: every lighting entry --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_every_mix(built_lib, oracle, entry):
    """322 x 190, all eight mixes: the entry on the packed planes == the checker on the widened planes, RGBA8 and radiance bits --
    reference as written / radius 0 / no ambient map, and Q fixes / a PCF radius / an ambient map; MIXED and all-half also with the
    cube chain (plus G0 half alone: the chain's quad exchange consumes G0 and G2, so a half plane on either side of it is run; the
    CPU tier runs the chain for all eight mixes).  Mix 0 is the fp32 kernels' own launch (no format bit)."""
    import torch
    from crychic_renderer_amd import Context, geometry as g
    W, H = 322, 190
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    L = _Lights(ctx, pl["consts"].pass_cb)
    dargs, chk = L.of(entry)
    rng = np.random.default_rng(11)
    ao = rng.integers(20000, 65535, (H // 2, W // 2), dtype=np.uint16)
    ao_dev = _to_dev(ctx, ao.view(np.int16))
    chain, levels = g.cube_mip_chain(p["cube"])
    chain_dev = _to_dev(ctx, chain)
    for mix in gf.MIXES:
        packed, d, wide = _packed_dev(ctx, p, dev, mix)
        for fixes, radius, with_ao, sky in ((0, 0.0, False, 1), (FIX_ALL, 0.01, True, 0)):
            rc, out, rad = _light(built_lib.lib, ctx, entry, L.cb, d, W, H, sky | fixes, radius=radius, ambient=ao_dev if with_ao else None, **dargs)
            built_lib.check(rc)
            torch.cuda.synchronize()
            ref = _checker(oracle, entry, L.pcb, wide, ao if with_ao else None, 3, radius, sky | fixes, chk)
            _assert_same(out, rad, ref, (entry, hex(mix), fixes))
        if mix in (gf.MIXED, gf.ALL_F16, gf.G0_F16):
            flags = 1 | ((levels & 15) << 16)
            rc, out, rad = _light(built_lib.lib, ctx, entry, L.cb, d, W, H, flags, radius=0.01, cube=chain_dev, **dargs)
            built_lib.check(rc)
            torch.cuda.synchronize()
            ref = _checker(oracle, entry, L.pcb, dict(wide, cube=chain), None, 3, 0.01, flags, chk, cube_dim=32)
            _assert_same(out, rad, ref, (entry, hex(mix), "chain"))
    ctx.close()


@pytest.mark.parametrize("mix", [gf.MIXED, gf.ALL_F16], ids=["mixed", "f16"])
def test_1080p_whole_frame_and_strips(built_lib, oracle, mix):
    """1920 x 1080 through crychic_deferred_light_point_shadows with every kind of local light and shadow, and through
    crychic_deferred_light without any: the whole frame == the checker on the widened planes, and two strips == the whole frame.
    These two entries are the two kernels of the general family (launch_light_general): the _points, _spots and _spots_shadowed entries
    launch the very light_general_local_kernel that _point_shadows does, with counts of 0, and all five entries are held against the
    checker at 322 x 190 (test_every_entry_every_mix); at this size the other six mixes are left to that test too."""
    import torch
    from crychic_renderer_amd import Context
    W, H = 1920, 1080
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    L = _Lights(ctx, pl["consts"].pass_cb, map_dim=128, cube_dim=256)
    packed, d, wide = _packed_dev(ctx, p, dev, mix)
    for entry in ("point_shadows", "light"):
        dargs, chk = L.of(entry)
        rc, out, rad = _light(built_lib.lib, ctx, entry, L.cb, d, W, H, 1, radius=0.01, **dargs)
        built_lib.check(rc)
        torch.cuda.synchronize()
        ref = _checker(oracle, entry, L.pcb, wide, None, 3, 0.01, 1, chk)
        _assert_same(out, rad, ref, (entry, "whole"))
        out2, rad2 = torch.zeros_like(out), torch.zeros_like(rad)
        for r0, rn in ((0, 538), (538, H - 538)):
            built_lib.check(_light(built_lib.lib, ctx, entry, L.cb, d, W, H, 1, radius=0.01, row0=r0, rows=rn, out=out2, rad=rad2, **dargs)[0])
        torch.cuda.synchronize()
        assert torch.equal(out2, out) and torch.equal(rad2.view(torch.int32), rad.view(torch.int32)), entry
    ctx.close()


# ---- statement 2: the producers ---------------------------------------------------------------------------------------------------

def test_draw_gbuffer_formats_matches_host_harness(built_lib, oracle):
    """crychic_draw_gbuffer_formats on the device == the host harness for MIXED, all-half and a mix with G0 half: normal_dev NULL and
    not, whole frame and a row range (texels outside it untouched).  With gbufferFlags 0 it equals today's four entries byte for
    byte."""
    import torch
    from crychic_renderer_amd import Context, SceneGeometry, geometry as g
    from crychic_renderer_amd.renderer import _ptr, _stream
    W, H = 322, 190
    ctx = Context(0)
    cs = scene_util.cpu_scene(W, H, 128, 16)["consts"]
    items, mats, tex = g.cascade_scene_items(), g.reference_materials(), g.procedural_textures(32)
    geo = SceneGeometry(ctx, items, mats, tex)
    view = np.array(cs.pass_cb.View, np.float32); vp = np.array(cs.pass_cb.ViewProj, np.float32)
    host = hostsim_lib.load()

    def planes(mix, fill=0xCD):
        """G0..G2 in the formats of mix, depth and the normal map, every byte `fill`."""
        def filled(nbytes, dtype):
            return torch.full((H, W, nbytes), fill, dtype=torch.uint8, device=ctx.device).view(dtype)
        gb = [filled(8, torch.float16) if mix & (gf.G0_F16 << k) else filled(16, torch.float32) for k in range(3)]
        return gb, filled(4, torch.int32).reshape(H, W), filled(8, torch.float16)

    def raw(t):
        return t.cpu().contiguous().view(torch.uint8).numpy()

    for mix in (gf.MIXED, gf.ALL_F16, gf.G0_F16 | gf.G2_F16):
        for fused in (False, True):
            for g_rows in (None, (40, 102)):
                gb, depth, normal = planes(mix)
                if fused:
                    geo.DrawNormalsDepthAndGBuffer(cs.pass_cb, normal, gb, depth, g_rows=g_rows)
                else:
                    geo.DrawGBuffer(cs.pass_cb, gb, depth, g_rows=g_rows)
                torch.cuda.synchronize()
                r0, rn = g_rows or (0, 0)
                ref = host.rasterize(3 if fused else 2, view, vp, items, mats, tex, W, H, mix=mix, g_row0=r0, g_rows=rn, fill=0xCD)
                what = (hex(mix), fused, g_rows)
                for k in range(3):
                    assert gb[k].dtype == (torch.float16 if mix & (gf.G0_F16 << k) else torch.float32)
                    assert np.array_equal(raw(gb[k]), np.ascontiguousarray(ref["g%d" % k]).view(np.uint8).reshape(H, W, -1)), (what, k)
                assert np.array_equal(depth.cpu().numpy().view(np.uint32), ref["depth"]), what
                if fused:
                    assert np.array_equal(raw(normal), np.ascontiguousarray(ref["normal"]).view(np.uint8).reshape(H, W, -1)), what
    # gbufferFlags 0 == the existing entries
    lib = built_lib.lib
    ws = geo.workspace(W, H)
    for fused in (False, True):
        for g_rows in (None, (40, 102)):
            a, da, na = planes(0)
            b, db, nb = planes(0)
            if fused:
                geo.DrawNormalsDepthAndGBuffer(cs.pass_cb, na, a, da, g_rows=g_rows)
            else:
                geo.DrawGBuffer(cs.pass_cb, a, da, g_rows=g_rows)
            r0, rn = g_rows or (0, 0)
            built_lib.check(lib.crychic_draw_gbuffer_formats(ctx.handle, C.byref(cs.pass_cb), geo.items, len(geo.items), _ptr(geo.materials),
                                                             geo.n_materials, geo.textures, geo.n_textures, _ptr(nb if fused else None), _ptr(b[0]),
                                                             _ptr(b[1]), _ptr(b[2]), 0, _ptr(db), W, H, r0, rn, _ptr(ws), ws.numel(),
                                                             _stream(ctx.device)))
            torch.cuda.synchronize()
            for k in range(3):
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (fused, g_rows, k)
            assert torch.equal(da, db) and torch.equal(na.view(torch.int16), nb.view(torch.int16)), (fused, g_rows)
    ctx.close()


# ---- the whole path ---------------------------------------------------------------------------------------------------------------

def _produced_frame(ctx, built_lib, W, H, SD, formats, fused=True):
    """The reference scene produced and lit on the device through Crychic with the given G-buffer formats."""
    import torch
    from crychic_renderer_amd import Crychic, LIGHT_SKY, SceneGeometry, geometry as g, scene
    consts = raster_util.frame_constants(W, H, SD)
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials(), g.procedural_textures(64))
    sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    cube = scene.make_cubemap(32, ctx.device)
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), cube, shadow_dim=SD, gbuffer_formats=formats)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    cbs = []
    for k in range(4):
        cb = built_lib.PassConstants(); cb.ViewProj[:] = list(raster_util.light_viewproj_t(consts, k)); cbs.append(cb)
    sgeo.DrawSceneToShadowMaps(cbs, [app.mShadowMap.mShadowMap[k] for k in range(4)])
    if fused:
        geo.DrawNormalsDepthAndGBuffer(app.mMainPassCB, app.mSsao.mNormalMap, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    else:
        geo.DrawNormalsAndDepth(app.mMainPassCB, app.mSsao.mNormalMap, app.mDepthStencilBuffer)
        geo.DrawGBuffer(app.mMainPassCB, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    app.blurCount, app.numDirLights, app.flags = 3, 1, LIGHT_SKY
    app.Draw()
    torch.cuda.synchronize()
    return app, consts, cube


def _app_planes(app, cube):
    g = [t.cpu().numpy() for t in app.mDeferred.mGBuffer]
    return {"g0": g[0], "g1": g[1], "g2": g[2], "depth": app.mDepthStencilBuffer.cpu().numpy().view(np.uint32),
            "shadow": np.stack([app.mShadowMap.mShadowMap[k].cpu().numpy().view(np.uint32) for k in range(4)]), "cube": cube.cpu().numpy(),
            "normal": app.mSsao.mNormalMap.cpu().numpy()}


def test_end_to_end_through_crychic(built_lib, oracle):
    """Producers -> SSAO -> blur -> lighting through Crychic with `mixed` and `f16`: the half planes are numpy.float16 of the fp32
    run's planes, the frame equals the oracle run on the planes the device produced, widened, the ambient map is the fp32 run's
    (SSAO does not read the G-buffer), strips give the whole frame, and set_gbuffer_formats / load_scene reach the same frame."""
    import torch
    from crychic_renderer_amd import Context
    W, H, SD = 320, 240, 512
    ctx = Context(0)
    base, consts, cube = _produced_frame(ctx, built_lib, W, H, SD, "f32")
    pb = _app_planes(base, cube)
    ao32 = base.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16).copy()
    frame32 = base.mBackBuffer.cpu().numpy().copy()
    scb = oracle_lib.as_oracle_cb(consts.ssao_cb, oracle_lib.OrSsaoConstants)
    pcb = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
    assert np.array_equal(ao32, oracle.compute_ssao(scb, pb["normal"], pb["depth"], consts.randvec, 3))
    for name, mix, fused in (("mixed", gf.MIXED, True), ("f16", gf.ALL_F16, False)):
        app, _, _ = _produced_frame(ctx, built_lib, W, H, SD, name, fused=fused)
        assert [app.mDeferred.Format(k) for k in range(3)] == [("f16" if mix & (gf.G0_F16 << k) else "f32") for k in range(3)]
        p = _app_planes(app, cube)
        assert gf.mix_of(p) == mix
        want = gf.pack_planes(pb, mix)
        for k in ("g0", "g1", "g2"):
            assert p[k].dtype == want[k].dtype and np.array_equal(p[k].view(np.uint16), want[k].view(np.uint16)), (name, k)
        for k in ("depth", "normal", "shadow"):
            assert np.array_equal(p[k].view(np.uint16), pb[k].view(np.uint16)), (name, k)
        ao = app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16).copy()
        assert np.array_equal(ao, ao32), name
        got = app.mBackBuffer.cpu().numpy().copy()
        wide = gf.widen_planes(p)
        ref = oracle.deferred_light(pcb, wide["g0"], wide["g1"], wide["g2"], wide["depth"], ao, wide["shadow"], wide["cube"], 1,
                                    app.pcfSearchRadius, sky=True)
        assert np.array_equal(got, ref), "%s: frame differs from the oracle in %d bytes" % (name, int((got != ref).sum()))
        assert not np.array_equal(got, frame32)                    # and it is not the fp32 frame: the rounding is visible somewhere
        app.mBackBuffer.zero_()
        for rank in range(3):
            r0, rn = C.c_uint32(), C.c_uint32()
            built_lib.check(built_lib.lib.crychic_strip_rows(H, 3, rank, C.byref(r0), C.byref(rn)))
            app.Draw(r0.value, rn.value)
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), got), name
        # the fp32 application switched over: load_scene converts the fp32 planes with torch's rounding
        base.set_gbuffer_formats(name)
        base.load_scene({"depth": base.mDepthStencilBuffer, "normal": base.mSsao.mNormalMap, "shadow": base.mShadowMap.mShadowMap,
                         "cube": cube, "randvec": base.mSsao.mRandomVectorMap, "consts": consts,
                         **{k: torch.from_numpy(pb[k]).to(ctx.device) for k in ("g0", "g1", "g2")}})
        base.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(base.mBackBuffer.cpu().numpy(), got), name
    ctx.close()


def test_4k_frame_all_half(built_lib, oracle):
    """One whole 3840 x 2160 frame (the benchmark's configuration: blurCount 4, 3 lights, 4 x 4096^2 cascades, 256^2 cube) with all
    three planes half4 against the oracle on the widened planes, byte for byte; the ambient map is the oracle's too."""
    import torch
    from crychic_renderer_amd import Context, Crychic, scene
    W, H = 3840, 2160
    ctx = Context(0)
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
    consts = planes["consts"]
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096, gbuffer_formats="f16")
    app.load_scene(planes)
    assert all(t.dtype == torch.float16 and t.numel() == W * H * 4 for t in app.mDeferred.mGBuffer)
    app.blurCount, app.numDirLights = 4, 3
    app.Draw()
    torch.cuda.synchronize()
    full = app.mBackBuffer.cpu().numpy()
    p = scene_util.np_planes(planes)
    wide = {k: app.mDeferred.mGBuffer[i].cpu().numpy().astype(np.float32) for i, k in enumerate(("g0", "g1", "g2"))}
    scb = oracle_lib.as_oracle_cb(consts.ssao_cb, oracle_lib.OrSsaoConstants)
    pcb = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
    ref_ao = oracle.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 4)
    assert np.array_equal(app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16), ref_ao)
    ref = oracle.deferred_light(pcb, wide["g0"], wide["g1"], wide["g2"], p["depth"], ref_ao, p["shadow"], p["cube"], 3, app.pcfSearchRadius)
    assert np.array_equal(full, ref), "frame differs in %d bytes" % int((full != ref).sum())
    ctx.close()


def test_mixed_frame_replays_from_a_hip_graph(built_lib, oracle):
    """A `mixed` frame captured into a hipGraph replays to the same bytes, and follows new contents of the captured half planes."""
    import torch
    from crychic_renderer_amd import Context
    W, H = 256, 256
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    app = _app(ctx, W, H, {k: v.clone() for k, v in dev.items()}, c)
    app.set_gbuffer_formats("mixed")
    app.load_scene({**{k: v.clone() for k, v in dev.items()}, "consts": c})
    assert [t.dtype for t in app.mDeferred.mGBuffer] == [torch.float32, torch.float16, torch.float16]
    app.blurCount, app.numDirLights = 3, 3
    app.Draw()                                   # code objects loaded before the capture
    torch.cuda.synchronize()
    direct = app.mBackBuffer.cpu().numpy().copy()
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    ao = oracle.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)

    def want(planes):
        w = gf.widen_planes(gf.pack_planes(planes, gf.MIXED))
        return oracle.deferred_light(pcb, w["g0"], w["g1"], w["g2"], w["depth"], ao, w["shadow"], w["cube"], 3, app.pcfSearchRadius, sky=True)

    assert np.array_equal(direct, want(p))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        app.Draw()
    app.mBackBuffer.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), direct)
    p2 = dict(p, g1=np.ascontiguousarray(p["g1"][:, ::-1]))     # another albedo plane in the captured half4 buffer
    app.mDeferred.mGBuffer[1].copy_(torch.from_numpy(p2["g1"]).to(ctx.device))
    for _ in range(2):
        app.mBackBuffer.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), want(p2))
    ctx.close()


# ---- the C++ veneer ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "f16"])
def test_veneer_set_gbuffer_format(built_lib, oracle, tmp_path, name):
    """tests/cpp/gbuffer_f16_driver: DeferredShading with R16G16B16A16 (and a format per plane) does not throw and sizes each plane,
    an unknown format still throws, and CRYCHIC::SetGBufferFormat + Draw on the built-in scene gives the planes and the back buffer
    of the Python path -- which equal the oracle on the widened planes."""
    import torch
    import test_cpp_veneer
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, SceneGeometry, geometry as g, scene
    exe = test_cpp_veneer.build_driver("gbuffer_f16_driver")
    W, H, SD, CD, BC, NL = 160, 120, 256, 32, 2, 1
    mix = {"mixed": gf.MIXED, "f16": gf.ALL_F16}[name]
    d = str(tmp_path)
    cube_np = scene.make_cubemap(CD, torch.device("cpu")).numpy()
    cube_np.tofile(d + "/cube.bin")
    r = subprocess.run([exe, d, str(W), str(H), str(SD), str(CD), str(BC), str(NL), name], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gbuffer f16 driver ok" in r.stdout and ("flags 0x%x" % mix) in r.stdout
    consts = raster_util.frame_constants(W, H, SD)
    C.memmove(C.addressof(consts.ssao_cb), open(d + "/ssao_cb.bin", "rb").read(), C.sizeof(consts.ssao_cb))
    C.memmove(C.addressof(consts.pass_cb), open(d + "/pass_cb.bin", "rb").read(), C.sizeof(consts.pass_cb))
    out = np.fromfile(d + "/out.bin", np.uint8).reshape(H, W, 4)
    dts = [np.float16 if mix & (gf.G0_F16 << k) else np.float32 for k in range(3)]
    gv = [np.fromfile(d + "/g%d_out.bin" % k, dts[k]).reshape(H, W, 4) for k in range(3)]
    # the Python path: the same scene (UpdateInstanceData culls against the frustum), the same constants
    ctx = Context(0)
    cam = scene.default_camera(W, H)
    geo = SceneGeometry(ctx, g.cascade_scene_items(cull_camera=cam), g.reference_materials(), None)
    sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True, cull_camera=cam))
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), torch.from_numpy(cube_np).to(ctx.device), shadow_dim=SD,
                  gbuffer_formats=name)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    cbs = []
    for k in range(4):
        cb = built_lib.PassConstants(); cb.ViewProj[:] = list(raster_util.light_viewproj_t(consts, k)); cbs.append(cb)
    sgeo.DrawSceneToShadowMaps(cbs, [app.mShadowMap.mShadowMap[k] for k in range(4)])
    geo.DrawNormalsDepthAndGBuffer(app.mMainPassCB, app.mSsao.mNormalMap, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    app.blurCount, app.numDirLights, app.flags = BC, NL, LIGHT_SKY
    app.Draw()
    torch.cuda.synchronize()
    for k in range(3):
        assert np.array_equal(app.mDeferred.mGBuffer[k].cpu().numpy().view(np.uint16), gv[k].view(np.uint16)), k
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), out)
    pcb = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
    ao = np.fromfile(d + "/ao.bin", np.uint16).reshape(H // 2, W // 2)
    depth = np.fromfile(d + "/depth_out.bin", np.uint32).reshape(H, W)
    shadow = np.stack([np.fromfile(d + "/shadow%d_out.bin" % k, np.uint32).reshape(SD, SD) for k in range(4)])
    ref = oracle.deferred_light(pcb, gv[0].astype(np.float32), gv[1].astype(np.float32), gv[2].astype(np.float32), depth, ao, shadow, cube_np,
                                NL, built_lib.lib.crychic_pcf_search_radius(SD, 1), sky=True)
    assert np.array_equal(out, ref)
    ctx.close()
