"""crychic_prefilter_cube_chain on the device against the checker (tests/gloss_ref) byte for byte, and what goes with it: the
canary past the chain, a side stream, a destination that is not 16-byte aligned, a captured graph, the refusals, and
Crychic.capture_environment(prefilter=True)."""
import ctypes as C

import numpy as np
import pytest

import gloss_lib
from test_gloss_host import SHAPES, checker_prefilter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gl():
    return gloss_lib.load()


@pytest.fixture(scope="module")
def ctx(built_lib):
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


def _device_prefilter(ctx, src, dim, levels, guard=256, misalign=0, stream=None):
    """crychic_prefilter_cube_chain of the flat chain `src` into a buffer pre-filled with 0xA5 that starts `misalign` bytes past an
    aligned address and has `guard` bytes past the chain."""
    import torch
    from crychic_renderer_amd import lib
    from crychic_renderer_amd._lib import check
    n = gloss_lib.chain_bytes(dim, levels)
    s = torch.from_numpy(np.ascontiguousarray(src[:n])).to(ctx.device)
    buf = torch.full((misalign + n + guard,), 0xA5, dtype=torch.uint8, device=ctx.device)
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(ctx.device) if stream is None else stream
    check(lib.crychic_prefilter_cube_chain(ctx.handle, C.c_void_p(s.data_ptr()), C.c_void_p(buf.data_ptr() + misalign), dim, levels,
                                           C.c_void_p(st.cuda_stream)))
    st.synchronize()
    out = buf.cpu().numpy()
    assert (out[:misalign] == 0xA5).all()
    return out[misalign:], n


@pytest.mark.parametrize("dim,levels", SHAPES)
def test_prefilter_equals_the_checker(ctx, gl, dim, levels):
    src, ref = checker_prefilter(gl, dim, levels)
    got, n = _device_prefilter(ctx, src, dim, levels)
    assert n == ref.size and np.array_equal(got[:n], ref)
    assert (got[n:] == 0xA5).all()


def test_prefilter_256_with_nine_levels(ctx, gl):
    src, ref = checker_prefilter(gl, 256, 9)
    got, n = _device_prefilter(ctx, src, 256, 9)
    assert np.array_equal(got[:n], ref) and (got[n:] == 0xA5).all()


def test_prefilter_into_a_destination_that_is_only_4_byte_aligned(ctx, gl):
    src, ref = checker_prefilter(gl, 20, 3)
    got, n = _device_prefilter(ctx, src, 20, 3, misalign=4)
    assert np.array_equal(got[:n], ref) and (got[n:] == 0xA5).all()


def test_prefilter_of_one_level_copies_it(ctx, gl):
    src, _ = checker_prefilter(gl, 8, 4)
    got, n = _device_prefilter(ctx, src, 8, 1)
    assert n == 6 * 8 * 8 * 4 and np.array_equal(got[:n], src[:n]) and (got[n:] == 0xA5).all()


def test_prefilter_runs_on_the_callers_stream(ctx, gl):
    """The source reaches its buffer on a side stream behind a few milliseconds of other work, and the prefilter is enqueued on that
    stream: launched on any other it would start at once and filter the 0xA5 fill."""
    import torch
    from crychic_renderer_amd import lib
    from crychic_renderer_amd._lib import check
    dim, levels = 16, 5
    src, ref = checker_prefilter(gl, dim, levels)
    host = torch.from_numpy(np.ascontiguousarray(src)).to(ctx.device)
    s = torch.full((src.size,), 0xA5, dtype=torch.uint8, device=ctx.device)
    dst = torch.zeros((src.size,), dtype=torch.uint8, device=ctx.device)
    ballast = torch.empty((1 << 28,), dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=ctx.device)
    with torch.cuda.stream(side):
        for k in range(16):
            ballast.fill_(k)
        s.copy_(host)
    check(lib.crychic_prefilter_cube_chain(ctx.handle, C.c_void_p(s.data_ptr()), C.c_void_p(dst.data_ptr()), dim, levels, C.c_void_p(side.cuda_stream)))
    side.synchronize()
    assert np.array_equal(dst.cpu().numpy(), ref)


def test_prefilter_captured_into_a_graph_and_replayed(ctx, gl):
    """Nothing is allocated or uploaded by the call: it is captured as it is, and a replay filters what the source holds then."""
    import torch
    from crychic_renderer_amd import lib
    from crychic_renderer_amd._lib import check
    dim, levels = 16, 5
    src, ref = checker_prefilter(gl, dim, levels)
    s = torch.zeros((src.size,), dtype=torch.uint8, device=ctx.device)
    dst = torch.zeros((src.size,), dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        check(lib.crychic_prefilter_cube_chain(ctx.handle, C.c_void_p(s.data_ptr()), C.c_void_p(dst.data_ptr()), dim, levels,
                                               C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)))
    s.copy_(torch.from_numpy(np.ascontiguousarray(src)).to(ctx.device))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), ref)


def test_prefilter_argument_errors(ctx):
    import torch
    from crychic_renderer_amd import lib
    n = int(lib.crychic_cube_chain_bytes(16, 5))
    buf = torch.full((2 * n + 64,), 0xA5, dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    a, b = buf.data_ptr(), buf.data_ptr() + n
    call = lambda s, d, dim=16, levels=5: lib.crychic_prefilter_cube_chain(ctx.handle, C.c_void_p(s), C.c_void_p(d), dim, levels, st)
    assert call(None, b) == -1 and call(a, None) == -1
    assert call(a, a) == -1 and b"overlap" in lib.crychic_last_error()
    assert call(a, b - 4) == -1 and call(a + 4, a) == -1            # one texel of overlap, either way round
    assert call(a, b, 0, 1) == -1 and call(a, b, 16, 0) == -1 and call(a, b, 16, 6) == -1
    assert b"6 cube map levels, a 16-texel face has at most 5" in lib.crychic_last_error()
    assert call(a + 2, b) == -1 and call(a, b + 2) == -1
    assert call(a, b, 16384, 2) == -4
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all()                        # nothing was enqueued by a refused call
    assert call(a, b) == 0
    torch.cuda.synchronize()


def test_python_prefilter_cube_map(ctx, gl):
    import torch
    from crychic_renderer_amd import Crychic, CrychicError
    dim, levels = 8, 4
    src, ref = checker_prefilter(gl, dim, levels)
    app = Crychic(ctx, 16, 16, torch.zeros((256, 256, 4), dtype=torch.uint8, device=ctx.device),
                  torch.zeros((6, 4, 4, 4), dtype=torch.uint8, device=ctx.device), shadow_dim=16)
    chain = torch.from_numpy(np.ascontiguousarray(src)).to(ctx.device)
    out = app.prefilter_cube_map(chain, dim, levels)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)
    again = app.prefilter_cube_map(chain, dim, levels, out=out)
    assert again is out
    with pytest.raises(CrychicError):
        app.prefilter_cube_map(chain, dim, levels, out=chain)
    with pytest.raises(CrychicError):
        app.prefilter_cube_map(chain, dim, levels, out=out[:-4])
    torch.cuda.synchronize()


# ---- the gloss lookup of the lighting pass on the device ---------------------------------------------------------------------------

from test_gloss_host import GLOSS, SIZES, gloss_chain, levels_flag, same_frame, with_edge_roughness

ENTRIES = ["light", "points", "spots", "spots_shadowed", "point_shadows"]


def _to_dev(ctx, a):
    import torch
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)       # torch wants a writable array
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(ctx.device)


def _dev_planes(ctx, p):
    return {k: _to_dev(ctx, p[k]) for k in ("g0", "g1", "g2", "depth", "shadow", "cube")}


def _call(lib, ctx, entry, cb, dev, W, H, flags, cube_dim, ndl=3, radius=0.0, points=(None, 0), spots=(None, 0), sdesc=None, pdesc=None,
          row0=0, rows=None, out=None, rad=None, stream=None):
    """One crychic_deferred_light* call with the arguments its entry takes; returns (status, RGBA8 tensor, radiance tensor)."""
    import torch
    from crychic_renderer_amd.renderer import _ptr, _stream
    rows = H - row0 if rows is None else rows
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device) if out is None else out
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device) if rad is None else rad
    sh = (C.c_void_p * 4)(*[dev["shadow"][k].data_ptr() for k in range(4)])
    args = [ctx.handle, C.byref(cb), _ptr(dev["g0"]), _ptr(dev["g1"]), _ptr(dev["g2"]), _ptr(dev["depth"]), None, sh, int(dev["shadow"].shape[-1]),
            _ptr(dev["cube"]), cube_dim, _ptr(out), _ptr(rad), W, H, row0, rows, ndl, radius, flags]
    st = _stream(ctx.device) if stream is None else stream
    sd, pd = (None if sdesc is None else C.byref(sdesc)), (None if pdesc is None else C.byref(pdesc))
    if entry == "light":
        rc = lib.crychic_deferred_light(*args, st)
    elif entry == "points":
        rc = lib.crychic_deferred_light_points(*args, _ptr(points[0]), points[1], st)
    elif entry == "spots":
        rc = lib.crychic_deferred_light_spots(*args, _ptr(points[0]), points[1], _ptr(spots[0]), spots[1], st)
    elif entry == "spots_shadowed":
        rc = lib.crychic_deferred_light_spots_shadowed(*args, _ptr(points[0]), points[1], _ptr(spots[0]), spots[1], sd, st)
    else:
        rc = lib.crychic_deferred_light_point_shadows(*args, _ptr(points[0]), points[1], _ptr(spots[0]), spots[1], sd, pd, st)
    return rc, out, rad


def _frames_equal(out, rad, ref):
    return same_frame((out.cpu().numpy(), rad.cpu().numpy()), ref)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_lighting_entry_with_the_flag_equals_the_checker(built_lib, ctx, gl, entry):
    """Each crychic_deferred_light* entry with CRYCHIC_LIGHT_CUBE_GLOSS == the checker, RGBA8 and radiance bits, at 64 x 48 (radius 0,
    5 levels) and 70 x 38 (radius > 0, Q fixes, 9 levels), with the roughness edge values and the lights the entry takes."""
    import torch
    from local_lights_util import FIX_ALL, _dev_lights
    from test_point_shadows import _frame_setup, _point_desc, _spot_desc
    for (W, H), radius, fixes, levels in zip(SIZES, (0.0, 0.01), (0, FIX_ALL), (5, 9)):
        p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, 2, 48, 3, seed=levels)
        chain, dim = gloss_chain(gl, p, levels)
        q = dict(with_edge_roughness(p, levels), cube=chain)
        dev = _dev_planes(ctx, q)
        flags = fixes | 1 | GLOSS | levels_flag(levels)
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
        ref = gl.checker_light(pcb, q, None, 3, radius, flags, cube_dim=dim, **kw)
        assert _frames_equal(out, rad, ref), (entry, W, H)


def test_gloss_on_a_half_float_mix_and_with_two_levels(built_lib, ctx, gl):
    import torch
    import gbuffer_f16_lib as gf
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    for levels, mix in ((2, 0), (5, gf.MIXED)):
        chain, dim = gloss_chain(gl, p, levels)
        packed = gf.pack_planes(dict(with_edge_roughness(p, levels), cube=chain), mix)
        wide = gf.widen_planes(packed)
        flags = 1 | GLOSS | levels_flag(levels)
        rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, packed), W, H, flags | mix, dim)
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, gl.checker_light(pcb, wide, None, 3, 0.0, flags, cube_dim=dim)), levels


def test_gloss_frame_in_three_row_strips_with_an_odd_row0(built_lib, ctx, gl):
    """320 x 180 lit as rows [0, 61), [61, 120), [120, 180): no quad is involved, so a strip may start on an odd row."""
    import torch
    from local_lights_util import _cpu
    W, H, levels = 320, 180, 5
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, levels)
    q = dict(with_edge_roughness(p, levels), cube=chain)
    dev = _dev_planes(ctx, q)
    flags = 1 | GLOSS | levels_flag(levels)
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    for r0, r1 in ((0, 61), (61, 120), (120, 180)):
        rc, _, _ = _call(built_lib.lib, ctx, "light", c.pass_cb, dev, W, H, flags, dim, row0=r0, rows=r1 - r0, out=out, rad=rad)
        built_lib.check(rc)
    torch.cuda.synchronize()
    assert _frames_equal(out, rad, gl.checker_light(pcb, q, None, 3, 0.0, flags, cube_dim=dim))


def test_gloss_frame_captured_into_a_graph_and_replayed(built_lib, ctx, gl):
    import torch
    from local_lights_util import _cpu
    W, H, levels = SIZES[0][0], SIZES[0][1], 5
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, levels)
    q = dict(with_edge_roughness(p, levels), cube=chain)
    dev = _dev_planes(ctx, q)
    flags = 1 | GLOSS | levels_flag(levels)
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
    assert _frames_equal(out, rad, gl.checker_light(pcb, q, None, 3, 0.0, flags, cube_dim=dim))


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_gloss_fuzz_planes_on_the_device(built_lib, ctx, gl, seed):
    import torch
    import fuzz_util
    import oracle_lib
    from crychic_renderer_amd import geometry as g
    W, H, planes, c, knobs = fuzz_util.random_case(seed, built_lib)
    chain, levels = g.cube_mip_chain(planes["cube"])
    dim = planes["cube"].shape[1]
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    q = dict(planes, cube=chain)
    flags = knobs["sky"] | GLOSS | levels_flag(levels)
    rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, q), W, H, flags, dim, ndl=knobs["numDirLights"],
                         radius=knobs["pcfSearchRadius"])
    built_lib.check(rc)
    torch.cuda.synchronize()
    assert _frames_equal(out, rad, gl.checker_light(pcb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim))


def test_the_flag_without_a_chain_is_refused(built_lib, ctx, gl):
    import torch
    from crychic_renderer_amd import Crychic, CrychicError
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, _ = _cpu(W, H)
    dev = _dev_planes(ctx, p)
    lib = built_lib.lib
    for flags in (GLOSS, GLOSS | 1, GLOSS | levels_flag(1)):
        rc, out, _ = _call(lib, ctx, "light", c.pass_cb, dev, W, H, flags, 32)
        assert rc == -1 and b"CRYCHIC_LIGHT_CUBE_GLOSS needs a chain" in lib.crychic_last_error()
        torch.cuda.synchronize()
        assert not out.any()
    app = Crychic(ctx, W, H, _to_dev(ctx, p["randvec"]), dev["cube"], shadow_dim=256)
    with pytest.raises(CrychicError):
        app.set_cube_map(dev["cube"], 32, 1, gloss=True)


@pytest.mark.parametrize("W,H", SIZES)
def test_hot_path_with_the_flag_equals_the_checker(built_lib, ctx, gl, W, H):
    """Crychic.Draw (crychic_draw_hot_path) with a gloss chain bound: the frame == the checker's, lit with the ambient map the device
    produced (the SSAO pass has its own tests)."""
    import torch
    from local_lights_util import _app, _cpu
    levels = 5
    pl, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, levels)
    q = dict(with_edge_roughness(p, levels), cube=chain)
    dev = {k: _to_dev(ctx, v) for k, v in q.items()}
    app = _app(ctx, W, H, dev, c)
    app.set_cube_map(dev["cube"], dim, levels, gloss=True)
    app.Draw()
    torch.cuda.synchronize()
    ao = app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16)
    ref = gl.checker_light(pcb, q, ao, 3, float(app.pcfSearchRadius), 1 | GLOSS | levels_flag(levels), cube_dim=dim)
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), ref[0])
    level0 = _app(ctx, W, H, dev, c)
    level0.set_cube_map(dev["cube"], dim, levels)          # the same chain through the derivative lookup: another frame
    level0.Draw()
    torch.cuda.synchronize()
    assert (level0.mBackBuffer.cpu().numpy() != ref[0]).any()


def test_capture_environment_with_prefilter(built_lib, ctx, gl):
    """capture_environment(prefilter=True) on the reference scene at dim 32 == the checker's prefilter of the captured box chain; the
    scratch chain is kept, so a second capture into `out` allocates nothing new."""
    import torch
    from test_env_capture import PROBE, SD, _Scene
    cap = _Scene(ctx)
    app = cap.app(ctx)
    box, dim, levels = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=32, shadow_dim=SD)
    torch.cuda.synchronize()
    box = box.cpu().numpy()
    assert (dim, levels) == (32, 6)
    pre, dim, levels = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=32, shadow_dim=SD, prefilter=True)
    torch.cuda.synchronize()
    ref = gl.prefilter(box, 32, 6)
    assert np.array_equal(pre.cpu().numpy(), ref) and (ref != box).any()
    scratch = app._probe_chains[(32, 6)]
    again, _, _ = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=32, shadow_dim=SD, prefilter=True, out=pre)
    torch.cuda.synchronize()
    assert again is pre and app._probe_chains[(32, 6)] is scratch and np.array_equal(pre.cpu().numpy(), ref)
    assert np.array_equal(scratch.cpu().numpy(), box)
    # a glossy owner: the probe's frames take the gloss lookup too (the capture of a glossy scene is glossy)
    app.set_cube_map(pre.clone(), 32, 6, gloss=True)
    glossy, _, _ = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=32, shadow_dim=SD)
    torch.cuda.synchronize()
    assert app._probes[(32, SD)].mCubeMapGloss and (glossy.cpu().numpy() != box).any()
