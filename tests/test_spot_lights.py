"""Spot lights (extension, include/crychic_hip.h crychic_deferred_light_spots): the reference's NUM_SPOT_LIGHTS branch
(PBR.hlsl:126-147) is dead code, so parity is against this repo's checker (tests/local_light_ref/local_light_ref.c, the frozen
oracle's or_light.c with the spot loop appended), which is itself anchored to the oracle (SpotPower 0 = a point light) and to an
independent float64 restatement."""
import ctypes as C

import numpy as np
import pytest

import hostsim_lib
import local_light_lib
import oracle_lib
from local_lights_util import (FIX_ALL, _app, _cpu, _dev_lights, _device_scene, as_or_lights, light_array, points_for_test,
                               run_local_lights_driver, spots_for_test)


# ---- CPU tier -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fixes", [0, FIX_ALL])
@pytest.mark.parametrize("chain", [False, True])
def test_checker_at_power_zero_is_the_oracles_point_light(oracle, fixes, chain):
    """SpotPower 0: pow(., 0) is exactly 1, so the checker's spot lights give the frozen oracle's point-light bits."""
    from crychic_renderer_amd import geometry as g
    W, H = 96, 64
    _, p, _, pcb = _cpu(W, H)
    kw, flags = {}, 1 | fixes
    if chain:
        cube, levels = g.cube_mip_chain(p["cube"])
        p = dict(p, cube=cube)
        kw = dict(cube_dim=32)
        flags |= (levels & 15) << 16
    sl = local_light_lib.load()
    spots, points = spots_for_test(power=0.0), points_for_test()
    # spots alone == the same lights as point lights
    got, grad = sl.checker(pcb, p, None, 3, 0.0, flags, spots=spots, **kw)
    ref, rref = oracle.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], None, p["shadow"], p["cube"], 3, 0.0, sky=True,
                                      want_radiance=True, point_lights=as_or_lights(spots), fixes=fixes,
                                      cube_levels=(flags >> 16) & 15, **kw)
    assert np.array_equal(got, ref) and np.array_equal(grad.view(np.uint32), rref.view(np.uint32))
    # points then spots == one point list in that order
    both = light_array(list(points) + list(spots))
    got, grad = sl.checker(pcb, p, None, 3, 0.0, flags, points=points, spots=spots, **kw)
    ref, rref = oracle.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], None, p["shadow"], p["cube"], 3, 0.0, sky=True,
                                      want_radiance=True, point_lights=as_or_lights(both), fixes=fixes,
                                      cube_levels=(flags >> 16) & 15, **kw)
    assert np.array_equal(got, ref) and np.array_equal(grad.view(np.uint32), rref.view(np.uint32))
    base = oracle.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], None, p["shadow"], p["cube"], 3, 0.0, sky=True,
                                 fixes=fixes, cube_levels=(flags >> 16) & 15, **kw)
    assert (got.astype(np.int32) - base.astype(np.int32)).max() > 20      # the lights really add light


def _spot_direct_f64(p, eye, lights):
    """Float64 restatement of the spot term (PBR.hlsl:126-147 enabled, quirks Q3 and Q4 as written): the sum over `lights` of
    brdf * Strength * nDotl * att per pixel and channel."""
    pi = 3.1415926
    g0, g1, g2 = (p[k].astype(np.float64) for k in ("g0", "g1", "g2"))
    pos, metal, alb, rough = g0[..., :3], g0[..., 3:4], g1[..., :3], g1[..., 3:4]
    unit = lambda v: v / np.sqrt((v * v).sum(-1, keepdims=True))
    dot = lambda a, b: (a * b).sum(-1, keepdims=True)
    n, v = unit(g2[..., :3]), unit(np.asarray(eye, np.float64) - pos)
    out = np.zeros(pos.shape, np.float64)
    for L in lights:
        l = np.asarray(L.Position[:], np.float64) - pos
        d = np.sqrt(dot(l, l))
        l = l / d
        att = np.clip((L.FalloffEnd - d) / (L.FalloffEnd - L.FalloffStart), 0.0, 1.0)
        att = att * np.maximum(dot(-np.asarray(L.Direction[:], np.float64), l), 0.001) ** L.SpotPower
        h = unit(v + l)
        hv, nl, nv = (np.maximum(dot(a, b), 0.001) for a, b in ((h, v), (n, l), (n, v)))
        a2 = rough * rough
        tt = np.maximum(dot(n, h), 0.001) ** 2 * (a2 - 1.0) + 1.0
        D = a2 / (pi * tt * tt)
        fr = np.clip(1.0 - hv, 0.0, 1.0) ** 5
        k = 0.125 * (rough + 1.0) ** 2
        G = nv / (nv * (1.0 - k) + k) * nl / (nl * (1.0 - k) + k)
        f0 = 0.04 + metal * (alb - 0.04)
        F = f0 + (1.0 - f0) * fr
        brdf = F * (0.25 * D * G * F / (nl * hv)) + (1.0 - F) * (1.0 - metal) * alb / pi
        out += np.where(d <= L.FalloffEnd, brdf * np.asarray(L.Strength[:], np.float64) * nl * att, 0.0)
    return out


def test_checker_matches_float64_restatement():
    """Powers 1, 8, 64 and 200, lights inside and outside their cones and lights that reach nothing: the checker's spot sum,
    recovered from its radiance, is the float64 restatement's within 2e-3 relative (+1e-5 absolute)."""
    W, H = 64, 48
    _, p, c, pcb = _cpu(W, H)
    sl = local_light_lib.load()
    spots = spots_for_test()
    assert sorted({s.SpotPower for s in spots}) == [1.0, 8.0, 64.0, 200.0]
    _, lit = sl.checker(pcb, p, None, 0, 0.0, 0, spots=spots)
    _, lit0 = sl.checker(pcb, p, None, 0, 0.0, 0)
    covered = (p["depth"] & 0xFFFFFF) < 0xFFFFFF
    # no directional or point light: lit - lit0 = (x / (x + 1))^(1 / 2.2) for the spot sum x, up to the float32 roundings of the
    # ambient and reflection terms added after it
    u = np.clip((lit[..., :3] - lit0[..., :3]).astype(np.float64), 0.0, None)
    t = u ** 2.2
    x = t / (1.0 - t)
    with np.errstate(invalid="ignore", divide="ignore"):                   # uncovered pixels have no normal
        ref = _spot_direct_f64(p, pcb.EyePosW[:], spots)
    m = covered[..., None] & (ref < 5.0)                                    # keep away from the tone map's flat end
    assert m.sum() > 0.5 * covered.sum() * 3
    err = np.abs(x - ref)[m]
    assert (err <= 2e-3 * ref[m] + 1e-5).all(), float((err / (ref[m] + 1e-5)).max())
    assert ref[m].max() > 0.1                                               # the lights reach the scene
    # the light that reaches nothing and the upward light's floor change nothing / almost nothing
    far = light_array([spots[3]])
    _, lit_far = sl.checker(pcb, p, None, 0, 0.0, 0, spots=far)
    assert np.array_equal(lit_far.view(np.uint32), lit0.view(np.uint32))


def test_det_pow_spot_range(oracle, hostsim):
    """det_pow (product, host build) == or_det_powf (oracle) bit for bit for x in [0.001, 1] and the spot powers.  Relative error
    against float64 below 1e-5 for y <= 64 wherever x^y >= 2^-125 (measured: 5.8e-6 at y = 64, 3.8e-7 at y = 1); below that, y * log2 x is clamped at -125 and the result is
    exactly 2^-125 (a spot factor of 2.4e-38 instead of a smaller one: no difference after the tone map)."""
    x = np.concatenate([np.linspace(0.001, 1.0, 20001, dtype=np.float32), np.float32([0.001, 0.5, 1.0])])
    for y in (0.0, 0.5, 1.0, 2.0, 8.0, 64.0, 200.0):
        yy = np.full_like(x, y)
        got = hostsim.eval_array(4, x, yy)
        ref = oracle.eval_array(4, x, yy)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), y
        if y == 0.0:
            assert (got == 1.0).all()                                       # the SpotPower 0 identity
        exact = x.astype(np.float64) ** y
        if y <= 64.0:
            inside = exact >= 2.0 ** -125                                   # below it the clamp holds the result at 2^-125
            rel = np.abs(got.astype(np.float64) - exact)[inside] / exact[inside]
            assert rel.max() < 1e-5, (y, rel.max())
        assert (got[exact < 2.0 ** -125] == np.float32(2.0 ** -125)).all()


@pytest.mark.parametrize("W,H", [(130, 70), (256, 144)])
def test_spot_kernel_body_matches_checker(built_lib, W, H):
    """The product's kernel body (light_core.hpp light_pixel with pbr_point_light then pbr_spot_light) on the host equals the
    checker bit for bit, mixed point and spot lists, with and without the Q fixes."""
    pl, p, c, pcb = _cpu(W, H)
    sl = local_light_lib.load()
    points, spots = points_for_test(), spots_for_test()
    for fixes, ndl, radius in ((0, 1, 0.0), (FIX_ALL, 3, 0.01)):
        got, grad = hostsim_lib.load().light_frame(c.pass_cb, p, None, ndl, radius, fixes | 1, points=points, spots=spots)
        ref, rref = sl.checker(pcb, p, None, ndl, radius, fixes | 1, points=points, spots=spots)
        assert np.array_equal(got, ref) and np.array_equal(grad.view(np.uint32), rref.view(np.uint32)), fixes
    base, _ = sl.checker(pcb, p, None, 1, 0.0, 1, points=points)
    assert (ref != base).any()


# ---- GPU tier -------------------------------------------------------------------------------------------------------------

def _light_spots(built_lib, ctx, c, dev, W, H, ambient, ndl, radius, flags, points, spots, row0=0, rows=None, out=None, rad=None,
                 cube=None, cube_dim=32):
    import torch
    from crychic_renderer_amd.renderer import _ptr, _stream
    rows = H - row0 if rows is None else rows
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device) if out is None else out
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device) if rad is None else rad
    sh = (C.c_void_p * 4)(*[dev["shadow"][k].data_ptr() for k in range(4)])
    pt, pn = points
    st, sn = spots
    rc = built_lib.lib.crychic_deferred_light_spots(ctx.handle, C.byref(c.pass_cb), _ptr(dev["g0"]), _ptr(dev["g1"]), _ptr(dev["g2"]),
                                                    _ptr(dev["depth"]), _ptr(ambient), sh, 256, _ptr(cube if cube is not None else dev["cube"]),
                                                    cube_dim, _ptr(out), _ptr(rad), W, H, row0, rows, ndl, radius, flags, _ptr(pt), pn,
                                                    _ptr(st), sn, _stream(ctx.device))
    return rc, out, rad


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(256, 144), (322, 190)])
def test_deferred_light_spots_on_device(built_lib, oracle, W, H):
    """crychic_deferred_light_spots == the checker bit for bit (RGBA8 and radiance): literal and intended PCF radius, with and
    without the ambient map, sky on, Q fixes, spots alone and points plus spots."""
    import torch
    from crychic_renderer_amd import Context
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    ao = oracle.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 2)
    ao_dev = torch.from_numpy(ao.view(np.int16)).to(ctx.device)
    sl = local_light_lib.load()
    points, spots = points_for_test(), spots_for_test()
    dp, ds = _dev_lights(ctx, points), _dev_lights(ctx, spots)
    cases = 0
    for radius_literal in (1, 0):
        radius = built_lib.lib.crychic_pcf_search_radius(256, radius_literal)
        for with_ao in (False, True):
            for with_points in (False, True):
                for fixes in (0, FIX_ALL):
                    rc, out, rad = _light_spots(built_lib, ctx, c, dev, W, H, ao_dev if with_ao else None, 3, radius, 1 | fixes,
                                                dp if with_points else (None, 0), ds)
                    built_lib.check(rc)
                    torch.cuda.synchronize()
                    ref, rref = sl.checker(pcb, p, ao if with_ao else None, 3, radius, 1 | fixes,
                                           points=points if with_points else None, spots=spots)
                    assert np.array_equal(out.cpu().numpy(), ref), (radius_literal, with_ao, with_points, fixes)
                    assert np.array_equal(rad.cpu().numpy().view(np.uint32), rref.view(np.uint32)), (radius_literal, with_ao, with_points, fixes)
                    cases += 1
    assert cases == 16
    ctx.close()


@pytest.mark.gpu
def test_deferred_light_spots_cube_chain_row_ranges(built_lib, oracle):
    """With the cube map's mip chain bound (quads inside wavefronts): the frame lit as even row ranges == the checker."""
    import torch
    from crychic_renderer_amd import Context, geometry as g
    W, H = 200, 120
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    chain, levels = g.cube_mip_chain(p["cube"])
    chain_dev = torch.from_numpy(chain).to(ctx.device)
    flags = 1 | ((levels & 15) << 16)
    points, spots = points_for_test(), spots_for_test()
    dp, ds = _dev_lights(ctx, points), _dev_lights(ctx, spots)
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    for r0, rn in ((0, 36), (36, 50), (86, 34)):
        built_lib.check(_light_spots(built_lib, ctx, c, dev, W, H, None, 3, 0.0, flags, dp, ds, r0, rn, out, rad, chain_dev)[0])
    torch.cuda.synchronize()
    ref, rref = local_light_lib.load().checker(pcb, dict(p, cube=chain), None, 3, 0.0, flags, points=points, spots=spots, cube_dim=32)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(rad.cpu().numpy().view(np.uint32), rref.view(np.uint32))
    # spots alone through the chain
    rc, out1, _ = _light_spots(built_lib, ctx, c, dev, W, H, None, 1, 0.0, flags, (None, 0), ds, cube=chain_dev)
    built_lib.check(rc)
    torch.cuda.synchronize()
    ref1, _ = local_light_lib.load().checker(pcb, dict(p, cube=chain), None, 1, 0.0, flags, spots=spots, cube_dim=32)
    assert np.array_equal(out1.cpu().numpy(), ref1)
    ctx.close()



@pytest.mark.gpu
def test_hot_path_spots_whole_strips_and_shared(built_lib, oracle):
    """crychic_draw_hot_path_spots with SSAO at blurCount 3 == the checker fed the oracle's ambient map; the frame drawn as
    several strips == the whole frame; crychic_draw_hot_path_shared_spots at one rank (1 and 3 parts) == the single-GPU frame."""
    import torch
    from crychic_renderer_amd import Context, sharding
    W, H = 256, 144
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    app = _app(ctx, W, H, dev, c)
    points, spots = points_for_test(), spots_for_test()
    app.set_point_lights(points)
    app.set_spot_lights(spots)
    app.Draw()
    torch.cuda.synchronize()
    full = app.mBackBuffer.cpu().numpy().copy()
    ao = oracle.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)
    assert np.array_equal(app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16), ao)
    ref, _ = local_light_lib.load().checker(pcb, p, ao, 3, app.pcfSearchRadius, 1, points=points, spots=spots)
    assert np.array_equal(full, ref)
    # strips
    app.mBackBuffer.zero_()
    for rank in range(3):
        r0, rn = C.c_uint32(), C.c_uint32()
        built_lib.check(built_lib.lib.crychic_strip_rows(H, 3, rank, C.byref(r0), C.byref(rn)))
        app.mSsao.mAmbientMap0.fill_(0x5A5A)
        app.Draw(r0.value, rn.value)
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), full)
    # the shared path at one rank
    ex = sharding.StripExchange(ctx, W, H, 1, 0, sharding.StripExchange.new_unique_id(), slots=1)
    for parts in (1, 3):
        app.mBackBuffer.zero_()
        app.Draw(shared=(ex.handle, None, parts))
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), full), parts
    ex.close()
    ctx.close()


@pytest.mark.gpu
def test_zero_spot_lights_change_nothing(built_lib):
    """numSpotLights = 0 through every new entry is byte-identical to the old entry (with and without point lights)."""
    import torch
    from crychic_renderer_amd import Context, sharding
    from crychic_renderer_amd.renderer import _ptr, _stream
    W, H = 192, 108
    lib = built_lib.lib
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    dp = _dev_lights(ctx, points_for_test())
    sh = (C.c_void_p * 4)(*[dev["shadow"][k].data_ptr() for k in range(4)])
    ex = sharding.StripExchange(ctx, W, H, 1, 0, sharding.StripExchange.new_unique_id(), slots=1)
    for pts in ((None, 0), dp):
        outs = []
        for new in (False, True):
            out = torch.full((H, W, 4), 7, dtype=torch.uint8, device=ctx.device)
            rad = torch.full((H, W, 4), 7.0, dtype=torch.float32, device=ctx.device)
            args = [ctx.handle, C.byref(c.pass_cb), _ptr(dev["g0"]), _ptr(dev["g1"]), _ptr(dev["g2"]), _ptr(dev["depth"]), None, sh, 256,
                    _ptr(dev["cube"]), 32, _ptr(out), _ptr(rad), W, H, 0, H, 3, 0.0, 1, _ptr(pts[0]), pts[1]]
            if new:
                built_lib.check(lib.crychic_deferred_light_spots(*args, None, 0, _stream(ctx.device)))
            else:
                built_lib.check(lib.crychic_deferred_light_points(*args, _stream(ctx.device)))
            torch.cuda.synchronize()
            outs.append((out.cpu().numpy(), rad.cpu().numpy().view(np.uint32)))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        app = _app(ctx, W, H, dev, c)
        app.set_point_lights(None if pts[1] == 0 else points_for_test())
        f = app.frame_desc()
        frames = []
        for entry in ("old", "spots", "shared", "shared_spots"):
            app.mBackBuffer.fill_(3)
            st = _stream(ctx.device)
            if entry == "old":
                built_lib.check(lib.crychic_draw_hot_path(ctx.handle, C.byref(app.mSsaoCB), C.byref(app.mMainPassCB), C.byref(f), st))
            elif entry == "spots":
                built_lib.check(lib.crychic_draw_hot_path_spots(ctx.handle, C.byref(app.mSsaoCB), C.byref(app.mMainPassCB), C.byref(f), None, 0, st))
            elif entry == "shared":
                built_lib.check(lib.crychic_draw_hot_path_shared(ex.handle, C.byref(app.mSsaoCB), C.byref(app.mMainPassCB), C.byref(f), None, 2, st))
            else:
                built_lib.check(lib.crychic_draw_hot_path_shared_spots(ex.handle, C.byref(app.mSsaoCB), C.byref(app.mMainPassCB), C.byref(f),
                                                                       None, 2, None, 0, st))
            torch.cuda.synchronize()
            frames.append(app.mBackBuffer.cpu().numpy().copy())
        for k in range(1, 4):
            assert np.array_equal(frames[0], frames[k]), k
    ex.close()
    ctx.close()


@pytest.mark.gpu
def test_spot_argument_errors(built_lib):
    """More than 1024 spot lights, or a null buffer with n > 0, is CRYCHIC_E_INVALID_ARG with a message, on every new entry."""
    import torch
    from crychic_renderer_amd import Context
    from crychic_renderer_amd.renderer import _ptr, _stream
    W, H = 64, 48
    lib = built_lib.lib
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    spots = torch.zeros((1025 * 48,), dtype=torch.uint8, device=ctx.device)
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    sh = (C.c_void_p * 4)(*[dev["shadow"][k].data_ptr() for k in range(4)])
    for buf, n in ((_ptr(spots), 1025), (None, 1)):
        rc = lib.crychic_deferred_light_spots(ctx.handle, C.byref(c.pass_cb), _ptr(dev["g0"]), _ptr(dev["g1"]), _ptr(dev["g2"]),
                                              _ptr(dev["depth"]), None, sh, 256, _ptr(dev["cube"]), 32, _ptr(out), None, W, H, 0, H, 1, 0.0, 0,
                                              None, 0, buf, n, _stream(ctx.device))
        assert rc == -1 and b"numSpotLights" in lib.crychic_last_error(), n
        app = _app(ctx, W, H, dev, c)
        f = app.frame_desc()
        rc = lib.crychic_draw_hot_path_spots(ctx.handle, C.byref(app.mSsaoCB), C.byref(app.mMainPassCB), C.byref(f), buf, n, _stream(ctx.device))
        assert rc == -1 and b"numSpotLights" in lib.crychic_last_error(), n
    torch.cuda.synchronize()
    assert not out.any()                                   # nothing was launched
    ctx.close()


@pytest.mark.gpu
def test_veneer_set_local_lights(built_lib, tmp_path):
    """tests/cpp/local_lights_driver.cpp renders through CRYCHIC::SetLocalLights; its frame equals the Python path's frame with the
    same planes and lights (and SetLocalLights(nullptr, 0, nullptr, 0) gives back the frame without local lights)."""
    import torch
    from crychic_renderer_amd import Context
    from local_lights_util import DRIVER_FRAME as F
    W, H, SD, CD, BC, NL = F["W"], F["H"], F["SD"], F["CD"], F["BC"], F["NL"]
    d = str(tmp_path)
    pl, _, points, spots, _ = run_local_lights_driver(d)
    out = np.fromfile(d + "/out.bin", dtype=np.uint8).reshape(H, W, 4)
    out0 = np.fromfile(d + "/out_nolights.bin", dtype=np.uint8).reshape(H, W, 4)
    ctx = Context(0)
    _, _, dev = _device_scene(ctx, W, H, SD, CD)
    # the veneer builds its own constant buffers (same builders, same camera) and its own random-vector map (same bytes)
    from crychic_renderer_amd._lib import PassConstants, SsaoConstants
    app = _app(ctx, W, H, dev, pl["consts"], blur=BC, ndl=NL)
    app.mMainPassCB, app.mSsaoCB = PassConstants(), SsaoConstants()
    C.memmove(C.addressof(app.mMainPassCB), open(d + "/pass_cb.bin", "rb").read(), C.sizeof(app.mMainPassCB))
    C.memmove(C.addressof(app.mSsaoCB), open(d + "/ssao_cb.bin", "rb").read(), C.sizeof(app.mSsaoCB))
    app.pcfSearchRadius = built_lib.lib.crychic_pcf_search_radius(SD, 1)
    app.set_point_lights(points)
    app.set_spot_lights(spots)
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(out, app.mBackBuffer.cpu().numpy())
    app.set_point_lights(None)
    app.set_spot_lights(None)
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(out0, app.mBackBuffer.cpu().numpy())
    assert not np.array_equal(out, out0)
    ctx.close()
