"""Shadowed spot lights (extension, include/crychic_hip.h crychic_deferred_light_spots_shadowed): the reference declares
gShadowMap[12] / gShadowTransforms[12] with slots 4..11 unused and leaves the spot branch's shadow factor commented out
(PBR.hlsl:145), so parity is against this repo's checker (tests/local_light_ref/local_light_ref.c, the frozen oracle's
or_light.c with the spot loop and a 9-tap CalcShadowFactor per light).  The checker is anchored to its own unshadowed frame (the
s = 1 transform), whose anchors are in tests/test_spot_lights.py, and to a float64 restatement of the factor."""
import ctypes as C
import math

import numpy as np
import pytest

import hostsim_lib
import local_light_lib
import oracle_lib
from local_lights_util import (FIX_ALL, _app, _cpu, _dev_lights, _device_scene, light_array, points_for_test, random_maps,
                               spot_transforms, spots_for_test, transposed, with_transforms)

CENTRE_T = np.zeros(16, np.float32)                       # every position -> map centre (0.5, 0.5) at depth 0: s = 1
CENTRE_T[3], CENTRE_T[7], CENTRE_T[15] = 0.5, 0.5, 1.0
FAR_T = CENTRE_T.copy()                                   # ... at depth 2: every comparison fails, s = 0
FAR_T[11] = 2.0


def _frame_setup(W, H, count, dim=64, seed=1):
    pl, p, c, _ = _cpu(W, H)
    spots = spots_for_test()
    T = [transposed(st) for _, _, st in spot_transforms(spots, count)]
    cb, pcb = with_transforms(c.pass_cb, T)
    return p, cb, pcb, spots, random_maps(count, dim, seed)


# ---- CPU tier: the checker's anchors -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fixes", [0, FIX_ALL])
def test_checker_unit_transform_is_the_unshadowed_frame(fixes):
    """Eight maps with a transform that sends every position to the map centre at depth 0 (s = 1 exactly) give the frame without
    maps bit for bit."""
    W, H = 96, 64
    _, p, c, _ = _cpu(W, H)
    spots, points = spots_for_test(), points_for_test()
    ll = local_light_lib.load()
    cb, pcb = with_transforms(c.pass_cb, [CENTRE_T] * 8)
    ref, rref = ll.checker(pcb, p, None, 3, 0.0, 1 | fixes, points=points, spots=spots)
    maps = random_maps(8, 32, 3)
    got, grad = ll.checker(pcb, p, None, 3, 0.0, 1 | fixes, points=points, spots=spots, maps=maps)
    assert np.array_equal(got, ref) and np.array_equal(grad.view(np.uint32), rref.view(np.uint32))


def _shadow_factor_f64(m, T, pos):
    """Float64 CalcShadowFactor (Common.hlsl:135-165) on a D24 map with gsamShadow (LESS_EQUAL per texel, then bilinear, border 0)."""
    dim = m.shape[0]
    d = (m & 0xFFFFFF).astype(np.float64) / 16777215.0
    sp = np.append(np.asarray(pos, np.float64), 1.0) @ np.asarray(T, np.float64).reshape(4, 4).T
    x, y, depth = sp[0] / sp[3], sp[1] / sp[3], sp[2] / sp[3]
    dx = 1.0 / dim
    tot = 0.0
    for oy in (-dx, 0.0, dx):
        for ox in (-dx, 0.0, dx):
            tx, ty = (x + ox) * dim - 0.5, (y + oy) * dim - 0.5
            i0, j0 = math.floor(tx), math.floor(ty)
            fx, fy = tx - i0, ty - j0
            def cmp(i, j):
                t = d[j, i] if 0 <= i < dim and 0 <= j < dim else 0.0
                return 1.0 if depth <= t else 0.0
            top = cmp(i0, j0) * (1 - fx) + cmp(i0 + 1, j0) * fx
            bot = cmp(i0, j0 + 1) * (1 - fx) + cmp(i0 + 1, j0 + 1) * fx
            tot += top * (1 - fy) + bot * fy
    return tot / 9.0


def test_checker_factor_matches_float64_restatement():
    """Random maps, perspective transforms and positions inside the light frusta: the checker's 9-tap factor is the float64
    CalcShadowFactor within 1e-5, and the product body's factor equals the checker's bit for bit."""
    rng = np.random.default_rng(7)
    ssl = local_light_lib.load()
    spots = spots_for_test()
    n, diffs = 0, []
    for k, (_, _, st) in enumerate(spot_transforms(spots, 8)):
        if k in (3,):
            continue                                             # the light 500 units away: its frustum misses the sample cube
        dim = int(rng.choice([16, 64, 257]))
        m = random_maps(1, dim, 100 + k)[0]
        T = transposed(st)
        L = spots[k]
        for _ in range(60):
            dist = rng.uniform(1.0, 0.9 * L.FalloffEnd)
            d = np.asarray(L.Direction[:], np.float64); d /= np.linalg.norm(d)
            pos = np.asarray(L.Position[:], np.float64) + dist * d + rng.uniform(-0.3, 0.3, 3) * dist
            pos = pos.astype(np.float32)
            s = ssl.factor(m, T, pos)
            assert np.float32(s).view(np.uint32) == np.float32(hostsim_lib.load().spot_shadow_factor(m, T, pos)).view(np.uint32)
            ref = _shadow_factor_f64(m, st.T.reshape(-1), pos.astype(np.float64))
            diffs.append(abs(s - ref))
            n += 1
            if not (0.0 < ref < 1.0):
                assert s == ref                                  # fully lit / fully shadowed: exact
    assert max(diffs) < 1e-5, max(diffs)
    assert n > 300


def test_factor_specials():
    """s == 1 at depth 0 and s == 0 at depth 2 for any map; a non-finite position addresses border texels only (s = 0: border
    0 fails LESS_EQUAL against a positive depth, and NaN fails it); positions behind the light are taken literally."""
    ssl = local_light_lib.load()
    m = random_maps(1, 32, 5)[0]
    for pos in ((1.0, 2.0, 3.0), (-7.5, 0.25, 40.0)):
        for factor in (ssl.factor, hostsim_lib.load().spot_shadow_factor):
            assert factor(m, CENTRE_T, pos) == 1.0
            assert factor(m, FAR_T, pos) == 0.0
    T = CENTRE_T.copy(); T[0] = 1.0; T[11] = 0.5                  # x = pos.x + 0.5, depth 0.5
    for pos in ((np.inf, 0.0, 0.0), (np.nan, 0.0, 0.0)):
        assert ssl.factor(m, T, pos) == 0.0 and hostsim_lib.load().spot_shadow_factor(m, T, pos) == 0.0
    spots = spots_for_test()
    _, _, st = spot_transforms(spots, 1)[0]
    L = spots[0]
    behind = np.asarray(L.Position[:], np.float32) - 3.0 * np.asarray(L.Direction[:], np.float32)
    T = transposed(st)
    a, b = ssl.factor(m, T, behind), hostsim_lib.load().spot_shadow_factor(m, T, behind)
    assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---- CPU tier: the product's kernel body --------------------------------------------------------------------------------------

@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("count", [1, 3, 8])
def test_shadowed_kernel_body_matches_checker(built_lib, chain, count):
    """light_core.hpp's body (pbr_spot_light with SpotShadowOf, built for the host) equals the checker bit for bit on random
    maps: Q3/Q4 switches off and on, both PCF radii, with and without the cube chain, points plus spots."""
    from crychic_renderer_amd import geometry as g
    W, H = 98, 66
    p, cb, pcb, spots, maps = _frame_setup(W, H, count, dim=48, seed=count)
    kw, extra = {}, 0
    if chain:
        cube, levels = g.cube_mip_chain(p["cube"])
        p = dict(p, cube=cube)
        kw, extra = dict(cube_dim=32), (levels & 15) << 16
    ssl = local_light_lib.load()
    points = points_for_test()
    for fixes, ndl, radius in ((0, 1, 0.0), (FIX_ALL, 3, 0.01)):
        flags = fixes | 1 | extra
        got, grad = hostsim_lib.load().light_frame(cb, p, None, ndl, radius, flags, points=points, spots=spots, maps=maps, **kw)
        ref, rref = ssl.checker(pcb, p, None, ndl, radius, flags, points=points, spots=spots, maps=maps, **kw)
        assert np.array_equal(got, ref) and np.array_equal(grad.view(np.uint32), rref.view(np.uint32)), fixes
        base, _ = ssl.checker(pcb, p, None, ndl, radius, flags, points=points, spots=spots, **kw)
        assert (ref != base).any()                                           # the shadows change the frame


# ---- CPU tier: the transform helper -------------------------------------------------------------------------------------------

def _look_at_f64(eye, at, up):
    z = at - eye; z /= np.linalg.norm(z)
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    V = np.zeros((4, 4))
    V[:3, 0], V[:3, 1], V[:3, 2] = x, y, z
    V[3, :3] = (-x @ eye, -y @ eye, -z @ eye)
    V[3, 3] = 1.0
    return V


def test_spot_shadow_transform_matches_float64():
    """crychic_update_spot_shadow_transform == LookAtLH * PerspectiveFovLH(fovY, 1, zNear, FalloffEnd) * T in float64 (1e-5
    relative to the matrix's scale); the up vector switches to +z for lights aimed (nearly) straight up or down; a point on the
    axis at any distance projects to the map centre (0.5, 0.5)."""
    spots = spots_for_test()
    spots[7].Direction[:] = (0.0, -1.0, 0.0)                               # straight down: up = (0, 0, 1)
    spots[8].Direction[:] = (0.01, 2.0, 0.0)                                # nearly straight up, not normalised
    tex = np.array([[0.5, 0, 0, 0], [0, -0.5, 0, 0], [0, 0, 1, 0], [0.5, 0.5, 0, 1]])
    for fov, zn in ((0.5 * math.pi, 0.5), (0.3, 2.0), (2.5, 0.1)):
        for k, (lv, lp, st) in enumerate(spot_transforms(spots, len(spots), fov, zn)):
            L = spots[k]
            pos, d = np.asarray(L.Position[:], np.float64), np.asarray(L.Direction[:], np.float64)
            up = np.array([0.0, 0.0, 1.0]) if abs(d[1]) > 0.999 * np.linalg.norm(d) else np.array([0.0, 1.0, 0.0])
            V = _look_at_f64(pos, pos + d, up)
            h = 1.0 / math.tan(0.5 * fov)
            P = np.zeros((4, 4)); P[0, 0] = P[1, 1] = h; P[2, 2] = L.FalloffEnd / (L.FalloffEnd - zn); P[2, 3] = 1.0
            P[3, 2] = -zn * L.FalloffEnd / (L.FalloffEnd - zn)
            for got, ref in ((lv, V), (lp, P), (st, V @ P @ tex)):
                assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (k, fov, zn)
            for dist in (zn, 1.0, 0.5 * L.FalloffEnd, L.FalloffEnd, 3.0 * L.FalloffEnd):
                q = np.append(pos + dist * d / np.linalg.norm(d), 1.0) @ st.astype(np.float64)
                tol = 4e-6 * (1.0 + np.linalg.norm(pos) + dist) / q[3]          # float32 matrix entries of size |pos|
                assert abs(q[0] / q[3] - 0.5) < tol and abs(q[1] / q[3] - 0.5) < tol, (k, dist)
            q = np.append(pos + zn * d / np.linalg.norm(d), 1.0) @ st.astype(np.float64)
            assert abs(q[2] / q[3]) < 1e-5 * (1.0 + np.linalg.norm(pos)) / zn                  # near plane -> depth 0
            q = np.append(pos + L.FalloffEnd * d / np.linalg.norm(d), 1.0) @ st.astype(np.float64)
            assert abs(q[2] / q[3] - 1.0) < 1e-5 * (1.0 + np.linalg.norm(pos)) / zn            # FalloffEnd -> depth 1


def test_spot_shadow_transform_argument_errors(built_lib):
    """Zero direction, fovY outside (0, pi), zNear <= 0, zNear >= FalloffEnd and NULL pointers are CRYCHIC_E_INVALID_ARG."""
    from crychic_renderer_amd import lib
    L = spots_for_test()[0]
    m = [(C.c_float * 16)() for _ in range(3)]
    ok = lambda light, fov=1.0, zn=0.5, mats=m: lib.crychic_update_spot_shadow_transform(light, fov, zn, *mats)
    assert ok(C.byref(L)) == 0
    Z = light_array([L])[0]
    Z.Direction[:] = (0.0, 0.0, 0.0)
    assert ok(C.byref(Z)) == -1
    for fov in (0.0, -0.5, math.pi, 4.0, float("nan")):
        assert ok(C.byref(L), fov=fov) == -1, fov
    for zn in (0.0, -1.0, L.FalloffEnd, L.FalloffEnd + 1.0, float("nan")):
        assert ok(C.byref(L), zn=zn) == -1, zn
    assert ok(None) == -1
    assert ok(C.byref(L), mats=[None, m[1], m[2]]) == -1


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------



def _desc(dev_maps, count=None):
    from crychic_renderer_amd._lib import SpotShadows
    d = SpotShadows()
    if dev_maps is None:
        return d
    d.count = dev_maps.shape[0] if count is None else count
    d.dim = dev_maps.shape[1]
    for k in range(dev_maps.shape[0]):
        d.maps[k] = dev_maps[k].data_ptr()
    return d


def _light(lib, ctx, cb, dev, W, H, flags, points, spots, desc, ndl=3, radius=0.0, ambient=None, row0=0, rows=None, out=None, rad=None,
           cube=None, shadowed=True):
    import torch
    from crychic_renderer_amd.renderer import _ptr, _stream
    rows = H - row0 if rows is None else rows
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev["g0"].device) if out is None else out
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=dev["g0"].device) if rad is None else rad
    sh = (C.c_void_p * 4)(*[dev["shadow"][k].data_ptr() for k in range(4)])
    args = [ctx.handle, C.byref(cb), _ptr(dev["g0"]), _ptr(dev["g1"]), _ptr(dev["g2"]), _ptr(dev["depth"]), _ptr(ambient), sh, 256,
            _ptr(cube if cube is not None else dev["cube"]), 32, _ptr(out), _ptr(rad), W, H, row0, rows, ndl, radius, flags,
            _ptr(points[0]), points[1], _ptr(spots[0]), spots[1]]
    if shadowed:
        rc = lib.crychic_deferred_light_spots_shadowed(*args, None if desc is None else C.byref(desc), _stream(ctx.device))
    else:
        rc = lib.crychic_deferred_light_spots(*args, _stream(ctx.device))
    return rc, out, rad


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(322, 190), (1920, 1080)])
def test_deferred_light_spots_shadowed_on_device(built_lib, W, H):
    """crychic_deferred_light_spots_shadowed == the checker bit for bit (RGBA8 and radiance) with 1, 3 and 8 shadowed lights:
    both PCF radii, Q fixes off and on, with and without point lights and the ambient map."""
    import torch
    from crychic_renderer_amd import Context
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    ssl = local_light_lib.load()
    points, spots = points_for_test(), spots_for_test()
    dp, ds = _dev_lights(ctx, points), _dev_lights(ctx, spots)
    rng = np.random.default_rng(11)
    ao = rng.integers(20000, 65535, (H // 2, W // 2), dtype=np.uint16)
    ao_dev = torch.from_numpy(ao.view(np.int16)).to(ctx.device)
    T = [transposed(st) for _, _, st in spot_transforms(spots, 8)]
    cb, pcb = with_transforms(pl["consts"].pass_cb, T)
    cases = 0
    for count, dim, fixes, radius, with_points, with_ao in ((1, 64, 0, 0.0, False, False), (3, 256, FIX_ALL, 0.01, True, True),
                                                             (8, 128, 0, 0.01, True, False), (8, 1024, FIX_ALL, 0.0, False, True)):
        maps = random_maps(count, dim, count + dim)
        mdev = torch.from_numpy(maps.view(np.int32)).to(ctx.device)
        rc, out, rad = _light(built_lib.lib, ctx, cb, dev, W, H, 1 | fixes, dp if with_points else (None, 0), ds, _desc(mdev),
                              radius=radius, ambient=ao_dev if with_ao else None)
        built_lib.check(rc)
        torch.cuda.synchronize()
        ref, rref = ssl.checker(pcb, p, ao if with_ao else None, 3, radius, 1 | fixes, points=points if with_points else None,
                                spots=spots, maps=maps)
        assert np.array_equal(out.cpu().numpy(), ref), (count, dim)
        assert np.array_equal(rad.cpu().numpy().view(np.uint32), rref.view(np.uint32)), (count, dim)
        base, _ = ssl.checker(pcb, p, ao if with_ao else None, 3, radius, 1 | fixes, points=points if with_points else None, spots=spots)
        assert (ref != base).any()
        cases += 1
    assert cases == 4
    ctx.close()


@pytest.mark.gpu
def test_shadowed_cube_chain_row_ranges(built_lib):
    """With the cube map's mip chain: the frame lit as even row ranges == the checker."""
    import torch
    from crychic_renderer_amd import Context, geometry as g
    W, H = 200, 120
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    spots = spots_for_test()
    T = [transposed(st) for _, _, st in spot_transforms(spots, 3)]
    cb, pcb = with_transforms(pl["consts"].pass_cb, T)
    chain, levels = g.cube_mip_chain(p["cube"])
    chain_dev = torch.from_numpy(chain).to(ctx.device)
    flags = 1 | ((levels & 15) << 16)
    maps = random_maps(3, 96, 2)
    mdev = torch.from_numpy(maps.view(np.int32)).to(ctx.device)
    ds = _dev_lights(ctx, spots)
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    for r0, rn in ((0, 36), (36, 50), (86, 34)):
        built_lib.check(_light(built_lib.lib, ctx, cb, dev, W, H, flags, (None, 0), ds, _desc(mdev), row0=r0, rows=rn, out=out, rad=rad,
                               cube=chain_dev)[0])
    torch.cuda.synchronize()
    ref, rref = local_light_lib.load().checker(pcb, dict(p, cube=chain), None, 3, 0.0, flags, spots=spots, maps=maps, cube_dim=32)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(rad.cpu().numpy().view(np.uint32), rref.view(np.uint32))
    ctx.close()


@pytest.mark.gpu
def test_shadowed_identities(built_lib):
    """Against the _spots entry: a NULL descriptor and count 0 are bit-identical; the s = 1 transform is bit-identical; the s = 0
    transform (depth 2) on the first k lights equals the frame with those k lights removed from the buffer."""
    import torch
    from crychic_renderer_amd import Context
    W, H = 256, 144
    lib = built_lib.lib
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    points, spots = points_for_test(), spots_for_test()
    dp, ds = _dev_lights(ctx, points), _dev_lights(ctx, spots)
    maps = torch.from_numpy(random_maps(8, 64, 9).view(np.int32)).to(ctx.device)
    pc = pl["consts"].pass_cb

    def frame(cb, spots_dev, desc, shadowed=True):
        rc, out, rad = _light(lib, ctx, cb, dev, W, H, 1, dp, spots_dev, desc, radius=0.01, shadowed=shadowed)
        built_lib.check(rc)
        torch.cuda.synchronize()
        return out.cpu().numpy(), rad.cpu().numpy().view(np.uint32)

    cbT = with_transforms(pc, [transposed(st) for _, _, st in spot_transforms(spots, 8)])[0]
    plain = frame(cbT, ds, None, shadowed=False)
    for d in (None, _desc(None), _desc(maps, count=0)):
        got = frame(cbT, ds, d)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    cbC = with_transforms(pc, [CENTRE_T] * 8)[0]
    got = frame(cbC, ds, _desc(maps))
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    for k in (1, 3, 8):
        cbF = with_transforms(pc, [FAR_T] * 8)[0]
        got = frame(cbF, ds, _desc(maps, count=k))
        rest = _dev_lights(ctx, light_array(list(spots)[k:]))
        ref = frame(cbF, rest, None, shadowed=False)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), k
        assert not np.array_equal(got[0], plain[0])
    ctx.close()



@pytest.mark.gpu
def test_hot_path_spots_shadowed_whole_strips_and_shared(built_lib, oracle):
    """crychic_draw_hot_path_spots_shadowed with SSAO == the checker fed the oracle's ambient map; strips == the whole frame;
    crychic_draw_hot_path_shared_spots_shadowed at one rank (1 and 3 parts) == the single-GPU frame.  Through Crychic.set_spot_shadows
    (maps filled by the caller)."""
    import torch
    from crychic_renderer_amd import Context, sharding
    W, H = 256, 144
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    app = _app(ctx, W, H, dev, c)
    points, spots = points_for_test(), spots_for_test()
    app.set_point_lights(points)
    app.set_spot_lights(spots)
    app.set_spot_shadows(3, dim=128)
    maps = random_maps(3, 128, 4)
    app.mSpotShadowMaps.copy_(torch.from_numpy(maps.view(np.int32)))
    app.Draw()
    torch.cuda.synchronize()
    full = app.mBackBuffer.cpu().numpy().copy()
    ao = oracle.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)
    T = [transposed(st) for _, _, st in spot_transforms(spots, 3)]
    _, pcb = with_transforms(c.pass_cb, T)
    ref, _ = local_light_lib.load().checker(pcb, p, ao, 3, app.pcfSearchRadius, 1, points=points, spots=spots, maps=maps)
    assert np.array_equal(full, ref)
    app.mBackBuffer.zero_()
    for rank in range(3):
        r0, rn = C.c_uint32(), C.c_uint32()
        built_lib.check(built_lib.lib.crychic_strip_rows(H, 3, rank, C.byref(r0), C.byref(rn)))
        app.Draw(r0.value, rn.value)
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), full)
    ex = sharding.StripExchange(ctx, W, H, 1, 0, sharding.StripExchange.new_unique_id(), slots=1)
    for parts in (1, 3):
        app.mBackBuffer.zero_()
        app.Draw(shared=(ex.handle, None, parts))
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), full), parts
    # count 0 through the shared and single entries == the _spots entries
    f = app.frame_desc()
    st = built_lib.lib
    from crychic_renderer_amd.renderer import _ptr, _stream
    frames = []
    for entry in ("spots", "spots_shadowed", "shared_spots", "shared_spots_shadowed"):
        app.mBackBuffer.fill_(3)
        a = (C.byref(app.mSsaoCB), C.byref(app.mMainPassCB), C.byref(f))
        if entry == "spots":
            built_lib.check(st.crychic_draw_hot_path_spots(ctx.handle, *a, _ptr(app.mSpotLights), len(spots), _stream(ctx.device)))
        elif entry == "spots_shadowed":
            built_lib.check(st.crychic_draw_hot_path_spots_shadowed(ctx.handle, *a, _ptr(app.mSpotLights), len(spots), None, _stream(ctx.device)))
        elif entry == "shared_spots":
            built_lib.check(st.crychic_draw_hot_path_shared_spots(ex.handle, *a, None, 2, _ptr(app.mSpotLights), len(spots), _stream(ctx.device)))
        else:
            d = _desc(None)
            built_lib.check(st.crychic_draw_hot_path_shared_spots_shadowed(ex.handle, *a, None, 2, _ptr(app.mSpotLights), len(spots), C.byref(d),
                                                                           _stream(ctx.device)))
        torch.cuda.synchronize()
        frames.append(app.mBackBuffer.cpu().numpy().copy())
    for k in range(1, 4):
        assert np.array_equal(frames[0], frames[k]), k
    ex.close()
    ctx.close()


@pytest.mark.gpu
def test_spot_shadow_argument_errors(built_lib):
    """count > 8, count > numSpotLights, a NULL map among the first count, dim 0 or 1 and dim > 16384 are CRYCHIC_E_INVALID_ARG with a
    message on every new entry, and nothing is launched."""
    import torch
    from crychic_renderer_amd import Context, sharding
    from crychic_renderer_amd.renderer import _ptr, _stream
    W, H = 64, 48
    lib = built_lib.lib
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    spots = spots_for_test()
    ds = _dev_lights(ctx, spots)
    maps = torch.zeros((8, 4, 4), dtype=torch.int32, device=ctx.device)
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    app = _app(ctx, W, H, dev, c)
    app.mBackBuffer.zero_()
    f = app.frame_desc()
    ex = sharding.StripExchange(ctx, W, H, 1, 0, sharding.StripExchange.new_unique_id(), slots=1)
    bad = []
    d = _desc(maps); d.count = 9; bad.append((d, ds))
    d = _desc(maps, count=3); bad.append((d, (ds[0], 2)))
    d = _desc(maps, count=3); d.maps[1] = None; bad.append((d, ds))
    d = _desc(maps, count=2); d.dim = 0; bad.append((d, ds))
    d = _desc(maps, count=2); d.dim = 1; bad.append((d, ds))
    d = _desc(maps, count=2); d.dim = 16385; bad.append((d, ds))
    for d, (sd, sn) in bad:
        rc, _, _ = _light(lib, ctx, c.pass_cb, dev, W, H, 0, (None, 0), (sd, sn), d, out=out, rad=None)
        assert rc == -1 and b"spot shadows" in lib.crychic_last_error()
        a = (C.byref(app.mSsaoCB), C.byref(app.mMainPassCB), C.byref(f))
        rc = lib.crychic_draw_hot_path_spots_shadowed(ctx.handle, *a, _ptr(sd), sn, C.byref(d), _stream(ctx.device))
        assert rc == -1 and b"spot shadows" in lib.crychic_last_error()
        rc = lib.crychic_draw_hot_path_shared_spots_shadowed(ex.handle, *a, None, 1, _ptr(sd), sn, C.byref(d), _stream(ctx.device))
        assert rc == -1 and b"spot shadows" in lib.crychic_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not app.mBackBuffer.any()
    ex.close()
    ctx.close()


def _scene_consts(W, H, SD):
    from crychic_renderer_amd import scene
    return scene.Constants(W, H, SD)


@pytest.mark.gpu
def test_perspective_producer_pass_matches_or_raster(built_lib, oracle):
    """A spot light's perspective pass (crychic_draw_scene_to_shadow_maps with ViewProj = lightView * lightProj) renders the
    reference scene bit-identically to oracle/or_raster.c, for the lights of scene.shadow_spot_lights and one aimed straight down;
    the eight maps of scene.shadow_spot_lights(8) in one call (two fused passes of four) equal eight single passes."""
    import torch
    from crychic_renderer_amd import Context, SceneGeometry, geometry as g, scene
    from crychic_renderer_amd._lib import PassConstants
    ctx = Context(0)
    sitems = g.cascade_scene_items(shadow_layer=True)
    sgeo = SceneGeometry(ctx, sitems)
    lights = light_array(list(scene.shadow_spot_lights(3)) + list(spots_for_test())[7:8])
    lights[3].Direction[:] = (0.0, -1.0, 0.0)
    lights[3].Position[:] = (2.0, 12.0, 1.0)
    view = np.eye(4, dtype=np.float32).reshape(-1)
    dim = 384
    cbs, planes, vps = [], [], []
    for lv, lp, _ in spot_transforms(lights, 4, 0.5 * math.pi, 0.5):
        vp = (lv @ lp).astype(np.float32).T.reshape(-1).copy()
        cb = PassConstants(); cb.ViewProj[:] = list(vp)
        cbs.append(cb); vps.append(vp)
        planes.append(torch.zeros((dim, dim), dtype=torch.int32, device=ctx.device))
    sgeo.DrawSceneToShadowMaps(cbs, planes)
    torch.cuda.synchronize()
    for k in range(4):
        ref = oracle_lib.rasterize(oracle, 0, view, vps[k], sitems, None, None, dim, dim, 10000, 2.0)["depth"]
        got = planes[k].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, ref), k
        assert (ref < 0xFFFFFF).mean() > 0.2, k                              # the light sees geometry
    eight = scene.shadow_spot_lights(8)
    cbs, fused, single = [], [], []
    for lv, lp, _ in spot_transforms(eight, 8, 0.5 * math.pi, 0.5):
        cb = PassConstants(); cb.ViewProj[:] = list((lv @ lp).astype(np.float32).T.reshape(-1))
        cbs.append(cb)
        fused.append(torch.zeros((256, 256), dtype=torch.int32, device=ctx.device))
        single.append(torch.zeros((256, 256), dtype=torch.int32, device=ctx.device))
    sgeo.DrawSceneToShadowMaps(cbs, fused)
    for k in range(8):
        sgeo.DrawSceneToShadowMap(cbs[k], single[k])
    torch.cuda.synchronize()
    for k in range(8):
        assert torch.equal(fused[k], single[k]), k
    ctx.close()


@pytest.mark.gpu
def test_reference_scene_shadowed_spot_end_to_end(built_lib, oracle):
    """The reference scene with a spot light aimed at a box (scene.shadow_spot_lights), everything produced on the device and the
    spot map rendered by Crychic.set_spot_shadows(geometry=...): the frame equals the checker fed the device's planes; pixels of
    the box's shadow on the grid get strictly less radiance than with count 0, and no pixel gets more."""
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, SceneGeometry, geometry as g, scene
    import raster_util
    W, H, SD = 320, 240, 512
    ctx = Context(0)
    consts = raster_util.frame_constants(W, H, SD)
    items, sitems = g.cascade_scene_items(), g.cascade_scene_items(shadow_layer=True)
    geo = SceneGeometry(ctx, items, g.reference_materials(), g.procedural_textures(64))
    sgeo = SceneGeometry(ctx, sitems)
    cube = scene.make_cubemap(32, ctx.device)
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), cube, shadow_dim=SD)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    cbs = []
    for k in range(4):
        cb = built_lib.PassConstants(); cb.ViewProj[:] = list(raster_util.light_viewproj_t(consts, k)); cbs.append(cb)
    sgeo.DrawSceneToShadowMaps(cbs, [app.mShadowMap.mShadowMap[k] for k in range(4)])
    geo.DrawNormalsDepthAndGBuffer(app.mMainPassCB, app.mSsao.mNormalMap, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    app.blurCount, app.numDirLights, app.flags = 3, 1, LIGHT_SKY
    lights = scene.shadow_spot_lights(1)
    app.set_spot_lights(lights)
    app.set_spot_shadows(1, dim=1024, geometry=sgeo)
    rad = {}
    for count in (1, 0):
        if count == 0:
            app.set_spot_shadows(0)
        app.Draw()
        torch.cuda.synchronize()
        rad[count] = app.mBackBuffer.cpu().numpy().copy()
    # the checker on the device's planes, with the device's spot map
    p = {"g0": app.mDeferred.mGBuffer[0].cpu().numpy(), "g1": app.mDeferred.mGBuffer[1].cpu().numpy(),
         "g2": app.mDeferred.mGBuffer[2].cpu().numpy(), "depth": app.mDepthStencilBuffer.cpu().numpy().view(np.uint32),
         "shadow": np.stack([app.mShadowMap.mShadowMap[k].cpu().numpy().view(np.uint32) for k in range(4)]),
         "cube": cube.cpu().numpy()}
    app.set_spot_shadows(1, dim=1024, geometry=sgeo)
    app.DrawSpotShadowMaps()
    torch.cuda.synchronize()
    maps = app.mSpotShadowMaps.cpu().numpy().view(np.uint32)
    ao = app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16)
    T = [transposed(st) for _, _, st in spot_transforms(lights, 1)]
    _, pcb = with_transforms(consts.pass_cb, T)
    ssl = local_light_lib.load()
    ref, lit1 = ssl.checker(pcb, p, ao, 1, app.pcfSearchRadius, 1, spots=lights, maps=maps)
    assert np.array_equal(rad[1], ref)
    _, lit0 = ssl.checker(pcb, p, ao, 1, app.pcfSearchRadius, 1, spots=lights)
    assert (lit1[..., :3] <= lit0[..., :3]).all()                               # a shadow never adds light
    darker = (lit1[..., :3] < lit0[..., :3]).all(-1)
    # the box's shadow on the grid: covered ground pixels (y ~ 0) that got darker
    ground = (np.abs(p["g0"][..., 1]) < 1e-3) & ((p["depth"] & 0xFFFFFF) < 0xFFFFFF)
    assert (darker & ground).sum() > 50, int((darker & ground).sum())
    assert not np.array_equal(rad[1], rad[0])
    ctx.close()
