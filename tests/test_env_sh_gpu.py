"""crychic_project_cube_sh and the lighting entries with CRYCHIC_LIGHT_AMBIENT_SH on the device against the checker (tests/env_sh_ref)
bit for bit: canaries round the tail, a tail of 0xFF and of the previous call's scratch, a side stream, a level of a chain, a captured
graph, every entry and Crychic.Draw, row strips, the fuzz planes, the refusals, and capture_environment(irradiance=True)."""
import ctypes as C

import numpy as np
import pytest

import env_sh_lib
from env_sh_lib import AMBIENT_SH, TAIL_BYTES, tail_offset, with_tail
from test_env_sh_host import (DIMS, bits, block_of, cube_for, edge_blocks, noise_level, scene_block, sh_flags, with_edge_normals)
from test_gloss_host import GLOSS, SIZES, levels_flag, same_frame, with_edge_roughness

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def es():
    return env_sh_lib.load()


@pytest.fixture(scope="module")
def ctx(built_lib):
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


def _project(ctx, buf, level_off, d, tail_off, stream=None):
    import torch
    from crychic_renderer_amd import lib
    from crychic_renderer_amd._lib import check
    st = torch.cuda.current_stream(ctx.device) if stream is None else stream
    check(lib.crychic_project_cube_sh(ctx.handle, C.c_void_p(buf.data_ptr() + level_off), d, C.c_void_p(buf.data_ptr() + tail_off),
                                      C.c_void_p(st.cuda_stream)))
    return st


def _buffer(ctx, level, fill):
    """[GUARD of 0xA5][level][padding of 0xA5 to 16][tail of `fill`][GUARD of 0xA5] on the device: (tensor, level offset, tail offset)."""
    import torch
    n = level.size
    toff = GUARD + (n + 15) // 16 * 16
    host = np.full(toff + TAIL_BYTES + GUARD, 0xA5, np.uint8)
    host[GUARD:GUARD + n] = level.reshape(-1)
    host[toff:toff + TAIL_BYTES] = fill
    buf = torch.from_numpy(host).to(ctx.device)
    assert buf.data_ptr() % 16 == 0
    return buf, host, GUARD, toff


def _check_tail(es, got, host, level, toff):
    """The coefficient block and the accumulators are the checker's, the reserved bytes of the tail and everything outside it are
    untouched."""
    ref = es.project(level)
    tail = got[toff:toff + TAIL_BYTES]
    assert np.array_equal(bits(block_of(tail)), bits(ref))
    assert np.array_equal(tail[144:368].view(np.int64), es.sums(level))
    keep = np.ones(got.size, bool)
    keep[toff:toff + 368] = False
    assert np.array_equal(got[keep], host[keep])


@pytest.mark.parametrize("d", DIMS + [256])
def test_projection_equals_the_checker(ctx, es, d):
    """Into a tail of 0xFF between 0xA5 canaries; then again into the same tail, which now holds the previous call's scratch: the
    same bits."""
    import torch
    level = noise_level(d)
    buf, host, loff, toff = _buffer(ctx, level, 0xFF)
    _project(ctx, buf, loff, d, toff).synchronize()
    first = buf.cpu().numpy()
    _check_tail(es, first, host, level, toff)
    _project(ctx, buf, loff, d, toff)
    _project(ctx, buf, loff, d, toff).synchronize()
    assert np.array_equal(buf.cpu().numpy(), first)
    torch.cuda.synchronize()


def test_projection_of_single_colour_cubes(ctx, es):
    for c in (0, 255):
        level = np.full((6, 16, 16, 4), c, np.uint8)
        buf, host, loff, toff = _buffer(ctx, level, 0x00)
        _project(ctx, buf, loff, 16, toff).synchronize()
        got = buf.cpu().numpy()
        _check_tail(es, got, host, level, toff)
        assert block_of(got[toff:toff + 144])[0, 0] == np.float32(c / 255.0)


def test_projection_of_level_2_of_a_chain_into_the_chains_own_tail(ctx, es):
    """dim 20, 3 levels: level 2 is 5 x 5 at byte 12000 of the chain, 4-byte but not 16-byte aligned from an odd multiple of 4; the tail
    sits at crychic_cube_sh_offset."""
    import torch
    from crychic_renderer_amd import geometry as g
    chain, levels = g.cube_mip_chain(noise_level(20), 3)
    assert levels == 3
    off2 = g.cube_chain_bytes(20, 2)
    toff = g.cube_sh_offset(20, 3)
    assert off2 == 12000 and toff == tail_offset(20, 3)
    host = np.full(4 + g.cube_chain_sh_bytes(20, 3) + GUARD, 0xA5, np.uint8)
    host[:chain.size] = chain
    buf = torch.from_numpy(host).to(ctx.device)
    _project(ctx, buf, off2, 5, toff).synchronize()
    level = chain[off2:off2 + 600].reshape(6, 5, 5, 4)
    _check_tail(es, buf.cpu().numpy(), host, level, toff)


def test_projection_runs_on_the_callers_stream(ctx, es):
    """The level reaches its buffer on a side stream behind other work and the projection is enqueued on that stream: launched on
    any other it would project the 0xA5 fill."""
    import torch
    d = 16
    level = noise_level(d)
    buf, host, loff, toff = _buffer(ctx, np.full_like(level, 0xA5), 0xFF)
    src = torch.from_numpy(level.reshape(-1)).to(ctx.device)
    ballast = torch.empty((1 << 28,), dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=ctx.device)
    with torch.cuda.stream(side):
        for k in range(16):
            ballast.fill_(k)
        buf[loff:loff + level.size].copy_(src)
    _project(ctx, buf, loff, d, toff, stream=side)
    side.synchronize()
    host[loff:loff + level.size] = level.reshape(-1)
    _check_tail(es, buf.cpu().numpy(), host, level, toff)


def test_projection_captured_into_a_graph_and_replayed(ctx, es):
    """Nothing is allocated or read back: the three launches are captured as they are, and a replay projects what the level holds
    then, twice over."""
    import torch
    d = 16
    level = noise_level(d, 5)
    buf, host, loff, toff = _buffer(ctx, np.zeros_like(level), 0xFF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _project(ctx, buf, loff, d, toff)
    buf[loff:loff + level.size].copy_(torch.from_numpy(level.reshape(-1)).to(ctx.device))
    host[loff:loff + level.size] = level.reshape(-1)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _check_tail(es, buf.cpu().numpy(), host, level, toff)


def test_projection_argument_errors(ctx):
    import torch
    from crychic_renderer_amd import lib
    d = 8
    n = 6 * d * d * 4
    buf = torch.full((n + TAIL_BYTES + 64,), 0xA5, dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    a, t = buf.data_ptr(), buf.data_ptr() + n
    call = lambda s, tail, dd=d: lib.crychic_project_cube_sh(ctx.handle, C.c_void_p(s), dd, C.c_void_p(tail), st)
    assert call(None, t) == -1 and call(a, None) == -1
    assert call(a, t, 0) == -1 and call(a, t, 8193) == -1
    assert call(a + 2, t) == -1 and b"4-byte" in lib.crychic_last_error()
    assert call(a, t + 4) == -1 and b"8-byte" in lib.crychic_last_error()
    assert call(a, t - 8) == -1 and b"overlaps" in lib.crychic_last_error()
    assert call(a, a) == -1 and call(a + TAIL_BYTES - 8, a) == -1
    assert call(a + TAIL_BYTES, a, 1) == 0                 # a 1 x 1 level right behind its tail
    torch.cuda.synchronize()
    assert (buf.cpu().numpy()[TAIL_BYTES + 24:] == 0xA5).all()          # the refused calls enqueued nothing
    assert call(a, t) == 0
    torch.cuda.synchronize()


# ---- the lighting pass on the device -------------------------------------------------------------------------------------------------

from test_gloss_gpu import ENTRIES, _call, _dev_planes, _frames_equal, _to_dev  # noqa: E402


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_lighting_entry_with_the_flag_equals_the_checker(built_lib, ctx, es, entry):
    """Each crychic_deferred_light* entry with CRYCHIC_LIGHT_AMBIENT_SH == the checker, RGBA8 and radiance bits: 64 x 48 with no chain
    and radius 0, 70 x 38 with a 5-level gloss chain, radius > 0 and the Q fixes; edge normals, edge roughness, an edge block."""
    import torch
    from local_lights_util import FIX_ALL, _dev_lights
    from test_point_shadows import _frame_setup, _point_desc, _spot_desc
    for (W, H), radius, fixes, levels, blk in zip(SIZES, (0.0, 0.01), (0, FIX_ALL), (0, 5), (0, 1)):
        p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, 2, 48, 3, seed=3 + levels)
        cube, dim = cube_for(es, p, levels)
        q = dict(with_edge_normals(with_edge_roughness(p, max(levels, 2))), cube=with_tail(cube, dim, levels, edge_blocks(es, p)[blk]))
        dev = _dev_planes(ctx, q)
        flags = fixes | 1 | sh_flags(levels)
        kw, dkw = {}, {}
        if entry != "light":
            kw["points"], dkw["points"] = points, _dev_lights(ctx, points)
        if entry in ("spots", "spots_shadowed", "point_shadows"):
            kw["spots"], dkw["spots"] = spots, _dev_lights(ctx, spots)
        if entry in ("spots_shadowed", "point_shadows"):
            mdev = _to_dev(ctx, maps)
            kw["maps"], dkw["sdesc"] = maps, _spot_desc(mdev)
        if entry == "point_shadows":
            cdev = _to_dev(ctx, cubes)
            kw["cubes"], kw["projs"], dkw["pdesc"] = cubes, projs, _point_desc(cdev, projs)
        rc, out, rad = _call(built_lib.lib, ctx, entry, cb, dev, W, H, flags, dim, radius=radius, **dkw)
        built_lib.check(rc)
        torch.cuda.synchronize()
        ref = es.checker_light(pcb, q, None, 3, radius, flags, cube_dim=dim, **kw)
        assert _frames_equal(out, rad, ref), (entry, W, H)


def test_edge_blocks_and_a_half_float_mix(built_lib, ctx, es):
    """Blocks that make e negative, NaN and infinite, on float planes; then the scene's block on a half-float mix, no chain and gloss."""
    import torch
    import gbuffer_f16_lib as gf
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    q0 = with_edge_normals(with_edge_roughness(p, 5))
    for k, block in enumerate(edge_blocks(es, p)):
        levels = (0, 2, 5)[k % 3]
        cube, dim = cube_for(es, p, levels)
        q = dict(q0, cube=with_tail(cube, dim, levels, block))
        flags = 1 | sh_flags(levels)
        rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, q), W, H, flags, dim, radius=(0.0, 0.01)[k & 1])
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, es.checker_light(pcb, q, None, 3, (0.0, 0.01)[k & 1], flags, cube_dim=dim)), k
    for levels in (0, 5):
        cube, dim = cube_for(es, p, levels)
        packed = gf.pack_planes(dict(q0, cube=with_tail(cube, dim, levels, scene_block(es, p))), gf.MIXED)
        wide = gf.widen_planes(packed)
        flags = 1 | sh_flags(levels)
        rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, packed), W, H, flags | gf.MIXED, dim)
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, es.checker_light(pcb, wide, None, 3, 0.0, flags, cube_dim=dim)), levels


def test_frame_in_three_row_strips_with_an_odd_row0(built_lib, ctx, es):
    """320 x 180 lit as rows [0, 61), [61, 120), [120, 180) equals the whole frame's checker; no chain and gloss."""
    import torch
    from local_lights_util import _cpu
    W, H = 320, 180
    _, p, c, pcb = _cpu(W, H)
    for levels in (0, 5):
        cube, dim = cube_for(es, p, levels)
        q = dict(with_edge_normals(with_edge_roughness(p, 5)), cube=with_tail(cube, dim, levels, scene_block(es, p)))
        dev = _dev_planes(ctx, q)
        flags = 1 | sh_flags(levels)
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
        rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
        for r0, r1 in ((0, 61), (61, 120), (120, 180)):
            rc, _, _ = _call(built_lib.lib, ctx, "light", c.pass_cb, dev, W, H, flags, dim, row0=r0, rows=r1 - r0, out=out, rad=rad)
            built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, es.checker_light(pcb, q, None, 3, 0.0, flags, cube_dim=dim)), levels


def test_frame_captured_into_a_graph_and_replayed(built_lib, ctx, es):
    import torch
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, pcb = _cpu(W, H)
    cube, dim = cube_for(es, p, 0)
    q = dict(with_edge_normals(p), cube=with_tail(cube, dim, 0, scene_block(es, p)))
    dev = _dev_planes(ctx, q)
    flags = 1 | AMBIENT_SH
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc, _, _ = _call(built_lib.lib, ctx, "light", c.pass_cb, dev, W, H, flags, dim, out=out, rad=rad,
                         stream=C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream))
        built_lib.check(rc)
    out.zero_(); rad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _frames_equal(out, rad, es.checker_light(pcb, q, None, 3, 0.0, flags, cube_dim=dim))


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_fuzz_planes_on_the_device(built_lib, ctx, es, seed):
    import torch
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
        rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, q), W, H, flags, dim, ndl=knobs["numDirLights"],
                             radius=knobs["pcfSearchRadius"])
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, es.checker_light(pcb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)), n


def test_refusals(built_lib, ctx, es):
    """The derivative-LOD chain with the flag is CRYCHIC_E_UNSUPPORTED with its message, a misaligned tail CRYCHIC_E_INVALID_ARG, both
    before anything is enqueued; set_cube_map refuses a tensor without room for the tail and the derivative chain."""
    import torch
    from crychic_renderer_amd import Crychic, CrychicError, geometry as g
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, _ = _cpu(W, H)
    chain, levels = g.cube_mip_chain(p["cube"])
    q = dict(p, cube=with_tail(chain, 32, levels, scene_block(es, p)))
    dev = _dev_planes(ctx, q)
    lib = built_lib.lib
    rc, out, _ = _call(lib, ctx, "light", c.pass_cb, dev, W, H, 1 | AMBIENT_SH | levels_flag(levels), 32)
    assert rc == -4 and b"CRYCHIC_LIGHT_AMBIENT_SH with a derivative-LOD chain" in lib.crychic_last_error()
    odd = dict(dev, cube=dev["cube"][2:])
    rc2, out2, _ = _call(lib, ctx, "light", c.pass_cb, odd, W, H, 1 | AMBIENT_SH, 32)
    assert rc2 == -1 and b"not 4-byte aligned" in lib.crychic_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not out2.any()
    app = Crychic(ctx, W, H, _to_dev(ctx, p["randvec"]), _to_dev(ctx, p["cube"]), shadow_dim=256)
    with pytest.raises(CrychicError):
        app.set_cube_map(_to_dev(ctx, p["cube"]), 32, 1, ambient_sh=True)                  # no room for the tail
    with pytest.raises(CrychicError):
        app.set_cube_map(dev["cube"][:-1], 32, levels, gloss=True, ambient_sh=True)        # one byte short
    with pytest.raises(CrychicError):
        app.set_cube_map(dev["cube"], 32, levels, ambient_sh=True)                         # the derivative chain
    app.set_cube_map(dev["cube"], 32, levels, gloss=True, ambient_sh=True)
    assert app.frame_desc().flags & AMBIENT_SH


@pytest.mark.parametrize("levels", [0, 5])
def test_hot_path_with_the_flag_equals_the_checker(built_lib, ctx, es, levels):
    """Crychic.project_irradiance into the chain's own tail, set_cube_map(ambient_sh=True) and Draw (crychic_draw_hot_path): the frame
    == the checker's, lit with the ambient map the device produced; and it differs from the constant-ambient frame."""
    import torch
    from crychic_renderer_amd import geometry as g
    from local_lights_util import _app, _cpu
    W, H = SIZES[1]
    pl, p, c, pcb = _cpu(W, H)
    cube, dim = cube_for(es, p, levels)
    q = with_edge_normals(with_edge_roughness(p, 5))
    host = with_tail(cube, dim, levels, np.zeros((9, 4), np.float32), fill=0xFF)
    dev = {k: _to_dev(ctx, v) for k, v in dict(q, cube=host).items()}
    app = _app(ctx, W, H, dev, c)
    assert app.project_irradiance(dev["cube"], dim, levels) is dev["cube"]
    app.set_cube_map(dev["cube"], dim, max(levels, 1), gloss=levels > 1, ambient_sh=True)
    app.Draw()
    torch.cuda.synchronize()
    tail = dev["cube"].cpu().numpy()[g.cube_sh_offset(dim, levels):]
    level0 = np.ascontiguousarray(cube[:6 * dim * dim * 4]).reshape(6, dim, dim, 4)
    assert np.array_equal(bits(block_of(tail)), bits(es.project(level0)))
    ao = app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16)
    ref = es.checker_light(pcb, dict(q, cube=with_tail(cube, dim, levels, es.project(level0))), ao, 3, float(app.pcfSearchRadius),
                           1 | sh_flags(levels), cube_dim=dim)
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), ref[0])
    const = _app(ctx, W, H, dev, c)
    const.set_cube_map(dev["cube"], dim, max(levels, 1), gloss=levels > 1)
    const.Draw()
    torch.cuda.synchronize()
    assert (const.mBackBuffer.cpu().numpy() != ref[0]).any()


def test_capture_environment_with_irradiance(built_lib, ctx, es):
    """capture_environment(irradiance=True), without and with prefilter=True, leaves a tail equal to the checker's projection of the
    captured level 0; a frame lit with that tail differs from the constant-ambient frame; the probe inherits the owner's state."""
    import torch
    from crychic_renderer_amd import CrychicError, geometry as g
    from test_env_capture import PROBE, SD, _Scene
    cap = _Scene(ctx)
    app = cap.app(ctx)
    dim = 32
    for pre in (False, True):
        chain, d, levels = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, prefilter=pre, irradiance=True)
        torch.cuda.synchronize()
        got = chain.cpu().numpy()
        assert (d, levels) == (dim, 6) and got.size == g.cube_chain_sh_bytes(dim, levels)
        level0 = got[:6 * dim * dim * 4].reshape(6, dim, dim, 4)
        off = g.cube_sh_offset(dim, levels)
        assert np.array_equal(bits(block_of(got[off:])), bits(es.project(level0))), pre
        assert block_of(got[off:])[0, :3].min() > 0.0
    with pytest.raises(CrychicError):
        app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, irradiance=True, out=chain[:-1])
    # the prefiltered chain with its tail, bound: the frame differs from the one with the constant ambient term
    import raster_util
    from crychic_renderer_amd import LIGHT_SKY
    app.flags = LIGHT_SKY
    cbs = []
    for k in range(4):
        cb = built_lib.PassConstants()
        cb.ViewProj[:] = list(raster_util.light_viewproj_t(cap.consts, k))
        cbs.append(cb)
    cap.shadow_geo.DrawSceneToShadowMaps(cbs, [app.mShadowMap.Resource(k) for k in range(4)])
    cap.geo.DrawNormalsDepthAndGBuffer(cap.consts.pass_cb, app.mSsao.mNormalMap, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    app.set_cube_map(chain, dim, levels, gloss=True)
    app.Draw()
    torch.cuda.synchronize()
    const = app.mBackBuffer.cpu().numpy().copy()
    app.set_cube_map(chain, dim, levels, gloss=True, ambient_sh=True)
    app.Draw()
    torch.cuda.synchronize()
    assert (app.mBackBuffer.cpu().numpy() != const).any()
    again, _, _ = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD)
    torch.cuda.synchronize()
    assert app._probes[(dim, SD)].mCubeMapAmbientSH and app._probes[(dim, SD)].mCubeMapGloss
