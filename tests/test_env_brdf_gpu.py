"""crychic_build_env_brdf and the lighting entries with CRYCHIC_LIGHT_ENV_BRDF on the device against the checker (tests/env_brdf_ref) bit
for bit: canaries round the table, a destination of 0xFF and of the previous call's output, a 4-byte aligned destination, a side
stream, a captured graph, every entry and Crychic.Draw, row strips, the fuzz planes, the refusals, and
capture_environment(prefilter=True, env_brdf=True)."""
import ctypes as C

import numpy as np
import pytest

import env_brdf_lib
import env_sh_lib
import gloss_lib
from env_brdf_lib import ENV_BRDF, TABLE_BYTES, table_offset, with_table
from env_sh_lib import AMBIENT_SH
from test_env_brdf_host import eye_of, random_table, spec_flags, with_table_roughness, with_view_normals
from test_env_sh_host import scene_block
from test_gloss_host import GLOSS, SIZES, gloss_chain, levels_flag

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def eb():
    return env_brdf_lib.load()


@pytest.fixture(scope="module")
def es():
    return env_sh_lib.load()


@pytest.fixture(scope="module")
def gl():
    return gloss_lib.load()


@pytest.fixture(scope="module")
def ctx(built_lib):
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


def _build(ctx, buf, off, stream=None):
    import torch
    from crychic_renderer_amd import lib
    from crychic_renderer_amd._lib import check
    st = torch.cuda.current_stream(ctx.device) if stream is None else stream
    check(lib.crychic_build_env_brdf(ctx.handle, C.c_void_p(buf.data_ptr() + off), C.c_void_p(st.cuda_stream)))
    return st


def _buffer(ctx, fill, shift=0):
    """[GUARD + shift of 0xA5][4096 bytes of `fill`][GUARD of 0xA5] on the device: (tensor, host copy, table offset)."""
    import torch
    off = GUARD + shift
    host = np.full(off + TABLE_BYTES + GUARD, 0xA5, np.uint8)
    host[off:off + TABLE_BYTES] = fill
    buf = torch.from_numpy(host.copy()).to(ctx.device)
    assert buf.data_ptr() % 16 == 0
    return buf, host, off


def _check_table(eb, got, host, off):
    """The 1024 dwords are the checker's, everything outside them is untouched."""
    assert np.array_equal(got[off:off + TABLE_BYTES].view(np.uint32) if off % 4 == 0 else
                          np.frombuffer(got[off:off + TABLE_BYTES].tobytes(), np.uint32), eb.table()[0])
    keep = np.ones(got.size, bool)
    keep[off:off + TABLE_BYTES] = False
    assert np.array_equal(got[keep], host[keep])


def test_table_equals_the_checker_between_canaries_and_over_its_own_output(ctx, eb):
    """Into 0xFF bytes between 0xA5 canaries; then again, twice, over its own output: the same bits."""
    import torch
    buf, host, off = _buffer(ctx, 0xFF)
    _build(ctx, buf, off).synchronize()
    first = buf.cpu().numpy()
    _check_table(eb, first, host, off)
    _build(ctx, buf, off)
    _build(ctx, buf, off).synchronize()
    assert np.array_equal(buf.cpu().numpy(), first)
    torch.cuda.synchronize()


def test_table_at_a_destination_that_is_only_4_byte_aligned(ctx, eb):
    buf, host, off = _buffer(ctx, 0x00, shift=4)
    assert (buf.data_ptr() + off) % 8 == 4
    _build(ctx, buf, off).synchronize()
    _check_table(eb, buf.cpu().numpy(), host, off)


def test_table_runs_on_the_callers_stream(ctx, eb):
    """The destination is filled with 0xFF on a side stream behind other work and the build is enqueued on that stream: launched on any
    other it would be overwritten by the fill."""
    import torch
    buf, host, off = _buffer(ctx, 0x00)
    ballast = torch.empty((1 << 28,), dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=ctx.device)
    with torch.cuda.stream(side):
        for k in range(16):
            ballast.fill_(k)
        buf[off:off + TABLE_BYTES].fill_(0xFF)
    _build(ctx, buf, off, stream=side)
    side.synchronize()
    _check_table(eb, buf.cpu().numpy(), host, off)


def test_table_captured_into_a_graph_and_replayed(ctx, eb):
    """Nothing is allocated or read back: the launch is captured as it is, and each of two replays rebuilds the table over whatever
    the destination holds then."""
    import torch
    buf, host, off = _buffer(ctx, 0xFF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _build(ctx, buf, off)
    for fill in (0x00, 0x5A):
        buf[off:off + TABLE_BYTES].fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        _check_table(eb, buf.cpu().numpy(), host, off)


def test_table_argument_errors(ctx):
    import torch
    from crychic_renderer_amd import lib
    buf = torch.full((TABLE_BYTES + 64,), 0xA5, dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    a = buf.data_ptr()
    assert lib.crychic_build_env_brdf(ctx.handle, None, st) == -1
    for mis in (1, 2, 3):
        assert lib.crychic_build_env_brdf(ctx.handle, C.c_void_p(a + mis), st) == -1 and b"4-byte" in lib.crychic_last_error()
    assert lib.crychic_build_env_brdf(None, C.c_void_p(a), st) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all()                # the refused calls enqueued nothing


# ---- the lighting pass on the device -------------------------------------------------------------------------------------------------

from test_gloss_gpu import ENTRIES, _call, _dev_planes, _frames_equal, _to_dev  # noqa: E402


@pytest.mark.parametrize("sh", [False, True])
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_lighting_entry_with_the_flag_equals_the_checker(built_lib, ctx, eb, es, gl, entry, sh):
    """Each crychic_deferred_light* entry with CRYCHIC_LIGHT_ENV_BRDF == the checker, RGBA8 and radiance bits: 64 x 48 with a 2-level
    chain, radius 0 and the built table, 70 x 38 with a 5-level chain, radius > 0, the Q fixes and a table of random dwords; the
    roughness and normal edge values; without and with SH."""
    import torch
    from local_lights_util import FIX_ALL, _dev_lights
    from test_point_shadows import _frame_setup, _point_desc, _spot_desc
    for (W, H), radius, fixes, levels, table in zip(SIZES, (0.0, 0.01), (0, FIX_ALL), (2, 5), (eb.table()[0], random_table(9))):
        p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, 2, 48, 3, seed=3 + levels)
        chain, dim = gloss_chain(gl, p, levels)
        q = dict(with_view_normals(with_table_roughness(p, levels), eye_of(cb)), cube=with_table(chain, dim, levels, table, scene_block(es, p)))
        dev = _dev_planes(ctx, q)
        flags = fixes | 1 | spec_flags(levels, sh)
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
        ref = eb.checker_light(pcb, q, None, 3, radius, flags, cube_dim=dim, **kw)
        assert _frames_equal(out, rad, ref), (entry, W, H)


def test_a_half_float_mix_and_an_infinite_eye(built_lib, ctx, eb, es, gl):
    """The built table on a half-float mix, without and with SH; then float planes with an infinite EyePosW."""
    import torch
    import gbuffer_f16_lib as gf
    from local_lights_util import _cpu
    from test_env_brdf_host import with_eye
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    for levels, sh in ((2, True), (5, False)):
        chain, dim = gloss_chain(gl, p, levels)
        q = dict(with_view_normals(with_table_roughness(p, levels), eye_of(c.pass_cb)),
                 cube=with_table(chain, dim, levels, eb.table()[0], scene_block(es, p)))
        packed = gf.pack_planes(q, gf.MIXED)
        wide = gf.widen_planes(packed)
        flags = 1 | spec_flags(levels, sh)
        rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, packed), W, H, flags | gf.MIXED, dim)
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, eb.checker_light(pcb, wide, None, 3, 0.0, flags, cube_dim=dim)), levels
        cb2, pcb2 = with_eye(c.pass_cb, (np.inf, 3.0, -np.inf))
        rc, out, rad = _call(built_lib.lib, ctx, "light", cb2, _dev_planes(ctx, q), W, H, flags, dim, radius=0.01)
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, eb.checker_light(pcb2, q, None, 3, 0.01, flags, cube_dim=dim)), levels


def test_frame_in_three_row_strips_with_an_odd_row0(built_lib, ctx, eb, es, gl):
    """320 x 180 lit as rows [0, 61), [61, 120), [120, 180) equals the whole frame's checker; without and with SH."""
    import torch
    from local_lights_util import _cpu
    W, H = 320, 180
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, 5)
    q = dict(with_view_normals(with_table_roughness(p, 5), eye_of(c.pass_cb)), cube=with_table(chain, dim, 5, eb.table()[0], scene_block(es, p)))
    dev = _dev_planes(ctx, q)
    for sh in (False, True):
        flags = 1 | spec_flags(5, sh)
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
        rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
        for r0, r1 in ((0, 61), (61, 120), (120, 180)):
            rc, _, _ = _call(built_lib.lib, ctx, "light", c.pass_cb, dev, W, H, flags, dim, row0=r0, rows=r1 - r0, out=out, rad=rad)
            built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, eb.checker_light(pcb, q, None, 3, 0.0, flags, cube_dim=dim)), sh


def test_frame_captured_into_a_graph_and_replayed(built_lib, ctx, eb, es, gl):
    import torch
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, 5)
    q = dict(with_view_normals(p, eye_of(c.pass_cb)), cube=with_table(chain, dim, 5, eb.table()[0], scene_block(es, p)))
    dev = _dev_planes(ctx, q)
    flags = 1 | spec_flags(5, True)
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
    assert _frames_equal(out, rad, eb.checker_light(pcb, q, None, 3, 0.0, flags, cube_dim=dim))


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_fuzz_planes_on_the_device(built_lib, ctx, eb, es, seed):
    import torch
    import fuzz_util
    import oracle_lib
    from crychic_renderer_amd import geometry as g
    W, H, planes, c, knobs = fuzz_util.random_case(seed, built_lib)
    chain, levels = g.cube_mip_chain(planes["cube"])
    dim = planes["cube"].shape[1]
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    block = es.project(planes["cube"])
    for sh, table in ((False, eb.table()[0]), (True, random_table(seed))):
        q = dict(planes, cube=with_table(chain, dim, levels, table, block))
        flags = knobs["sky"] | spec_flags(levels, sh)
        rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, q), W, H, flags, dim, ndl=knobs["numDirLights"],
                             radius=knobs["pcfSearchRadius"])
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, eb.checker_light(pcb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)), sh


def test_refusals(built_lib, ctx, eb, es, gl):
    """The flag without CRYCHIC_LIGHT_CUBE_GLOSS or without a chain and a misaligned table are CRYCHIC_E_INVALID_ARG with their
    messages, before anything is enqueued; set_cube_map refuses a tensor without room for the table and the flag without gloss."""
    import torch
    from crychic_renderer_amd import Crychic, CrychicError
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, _ = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, 5)
    q = dict(p, cube=with_table(chain, dim, 5, eb.table()[0], scene_block(es, p)))
    dev = _dev_planes(ctx, q)
    lib = built_lib.lib
    outs = []
    for flags in (1 | ENV_BRDF | levels_flag(5), 1 | ENV_BRDF, 1 | ENV_BRDF | AMBIENT_SH):
        rc, out, _ = _call(lib, ctx, "light", c.pass_cb, dev, W, H, flags, dim)
        assert rc == -1 and b"CRYCHIC_LIGHT_ENV_BRDF needs a prefiltered chain" in lib.crychic_last_error(), hex(flags)
        outs.append(out)
    rc, out, _ = _call(lib, ctx, "light", c.pass_cb, dev, W, H, 1 | ENV_BRDF | GLOSS, dim)
    assert rc == -1 and b"needs a chain" in lib.crychic_last_error()
    outs.append(out)
    null = dict(dev, cube=None)
    rc, out, _ = _call(lib, ctx, "light", c.pass_cb, null, W, H, 1 | spec_flags(5), dim)
    assert rc == -1 and b"null argument" in lib.crychic_last_error()      # the entries' own test of their pointers comes first; the
    outs.append(out)                                                      # binding's message for it: tests/test_env_brdf_host.py
    odd = dict(dev, cube=dev["cube"][2:])
    rc, out, _ = _call(lib, ctx, "light", c.pass_cb, odd, W, H, 1 | spec_flags(5), dim)
    assert rc == -1 and b"CRYCHIC_LIGHT_ENV_BRDF: the table" in lib.crychic_last_error() and b"not 4-byte aligned" in lib.crychic_last_error()
    outs.append(out)
    torch.cuda.synchronize()
    assert not any(o.any() for o in outs)
    app = Crychic(ctx, W, H, _to_dev(ctx, p["randvec"]), _to_dev(ctx, p["cube"]), shadow_dim=256)
    with pytest.raises(CrychicError, match="env_brdf needs a tensor of"):
        app.set_cube_map(dev["cube"][:-1], dim, 5, gloss=True, env_brdf=True)            # one byte short
    with pytest.raises(CrychicError, match="env_brdf needs a tensor of"):
        app.set_cube_map(_to_dev(ctx, chain), dim, 5, gloss=True, env_brdf=True)          # no room for tail and table
    with pytest.raises(CrychicError, match="env_brdf needs a prefiltered chain"):
        app.set_cube_map(dev["cube"], dim, 5, env_brdf=True)                              # the flag without gloss
    assert not app.frame_desc().flags & ENV_BRDF
    app.set_cube_map(dev["cube"], dim, 5, gloss=True, env_brdf=True)
    assert app.frame_desc().flags & ENV_BRDF and not app.frame_desc().flags & AMBIENT_SH
    app.set_cube_map(dev["cube"], dim, 5, gloss=True, ambient_sh=True, env_brdf=True)
    assert app.frame_desc().flags & ENV_BRDF and app.frame_desc().flags & AMBIENT_SH


@pytest.mark.parametrize("sh", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_hot_path_with_the_flag_equals_the_checker(built_lib, ctx, eb, es, gl, W, H, sh):
    """Crychic.build_env_brdf into the chain's own tensor, set_cube_map(env_brdf=True) and Draw (crychic_draw_hot_path): the frame == the
    checker's, lit with the ambient map the device produced; and it differs from the gloss frame.  Draw's cache key holds the state."""
    import torch
    from crychic_renderer_amd import geometry as g
    from local_lights_util import _app, _cpu
    pl, p, c, pcb = _cpu(W, H)
    levels = 5 if W == SIZES[1][0] else 2
    chain, dim = gloss_chain(gl, p, levels)
    q = with_view_normals(with_table_roughness(p, levels), eye_of(c.pass_cb))
    block = scene_block(es, p)
    host = with_table(chain, dim, levels, np.full(1024, 0xFFFFFFFF, np.uint32), block, fill=0xFF)
    dev = {k: _to_dev(ctx, v) for k, v in dict(q, cube=host).items()}
    app = _app(ctx, W, H, dev, c)
    app.set_cube_map(dev["cube"], dim, levels, gloss=True, ambient_sh=sh)
    app.Draw()
    torch.cuda.synchronize()
    gloss = app.mBackBuffer.cpu().numpy().copy()
    assert app.build_env_brdf(dev["cube"], dim, levels) is dev["cube"]
    app.set_cube_map(dev["cube"], dim, levels, gloss=True, ambient_sh=sh, env_brdf=True)
    app.Draw()
    torch.cuda.synchronize()
    got = dev["cube"].cpu().numpy()
    off = g.cube_env_brdf_offset(dim, levels)
    assert off == table_offset(dim, levels) and np.array_equal(got[off:off + TABLE_BYTES].view(np.uint32), eb.table()[0])
    assert np.array_equal(got[:off], host[:off])
    ao = app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16)
    ref = eb.checker_light(pcb, dict(q, cube=with_table(chain, dim, levels, eb.table()[0], block)), ao, 3, float(app.pcfSearchRadius),
                           1 | spec_flags(levels, sh), cube_dim=dim)
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), ref[0])
    assert (gloss != ref[0]).any()


def test_capture_environment_with_the_table(built_lib, ctx, eb, es):
    """capture_environment(prefilter=True, env_brdf=True), without and with irradiance=True, leaves the checker's table behind the
    chain; a frame lit with it differs from the gloss frame; env_brdf without prefilter is refused; the probe inherits the owner's
    state."""
    import torch
    from crychic_renderer_amd import CrychicError, geometry as g
    from test_env_capture import PROBE, SD, _Scene
    cap = _Scene(ctx)
    app = cap.app(ctx)
    dim = 32
    for irr in (False, True):
        chain, d, levels = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, prefilter=True, irradiance=irr,
                                                   env_brdf=True)
        torch.cuda.synchronize()
        got = chain.cpu().numpy()
        assert (d, levels) == (dim, 6) and got.size == g.cube_chain_env_bytes(dim, levels)
        off = g.cube_env_brdf_offset(dim, levels)
        assert np.array_equal(got[off:].view(np.uint32), eb.table()[0]), irr
        if irr:
            level0 = got[:6 * dim * dim * 4].reshape(6, dim, dim, 4)
            assert np.array_equal(got[off - 512:off - 512 + 144].view(np.uint32), es.project(level0).view(np.uint32).reshape(-1))
    with pytest.raises(CrychicError, match="env_brdf needs prefilter=True"):
        app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, env_brdf=True)
    with pytest.raises(CrychicError, match=r"env_brdf needs a chain \(levels > 1\)"):
        app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, levels=1, prefilter=True, env_brdf=True)
    with pytest.raises(CrychicError):
        app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, prefilter=True, env_brdf=True, out=chain[:-1])
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
    app.set_cube_map(chain, dim, levels, gloss=True, ambient_sh=True)
    app.Draw()
    torch.cuda.synchronize()
    gloss = app.mBackBuffer.cpu().numpy().copy()
    app.set_cube_map(chain, dim, levels, gloss=True, ambient_sh=True, env_brdf=True)
    app.Draw()
    torch.cuda.synchronize()
    assert (app.mBackBuffer.cpu().numpy() != gloss).any()
    again, _, _ = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD)
    torch.cuda.synchronize()
    probe = app._probes[(dim, SD)]
    assert probe.mCubeMapEnvBrdf and probe.mCubeMapAmbientSH and probe.mCubeMapGloss
