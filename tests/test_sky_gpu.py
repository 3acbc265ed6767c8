"""crychic_render_sky on the device: the kernel against the checker (tests/sky_ref) byte for byte on the corpus of the CPU tier, behind
guard bytes, on a misaligned plane and in face ranges; the refusals with a context; the call replayed from a graph; and the sky behind
Crychic.render_sky, Crychic.sky_sun_colour and Crychic.followSun."""
import ctypes as C

import numpy as np
import pytest

import sky_lib as sk
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu


def sky_params(lib, params):
    return None if params is None else lib.SkyParams.from_buffer_copy(sk.params_array(params).tobytes())


def run_device(dev, dim, params=None, face0=0, faces=6, misalign=0):
    """crychic_render_sky into a guarded device cube of 0xA5; returns it as numpy, the guards checked."""
    lib, ctx, torch = dev
    planes = DevicePlanes(dev)
    cube = planes.blank("cube", (6, dim, dim, 4), np.uint8, misalign)
    p = sky_params(lib, params)
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_render_sky(ctx.handle, C.c_void_p(cube.data_ptr()), dim, face0, faces, None if p is None else C.byref(p),
                                         C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return cube.cpu().numpy().reshape(6, dim, dim, 4)


@pytest.mark.parametrize("dim", sk.DIMS)
def test_device_equals_checker(dev, dim):
    ran = 0
    for name, d, params in sk.corpus():
        if d != dim:
            continue
        ref, _ = sk.expected(name)
        got = run_device(dev, dim, params, misalign=16 * (ran % 2))
        assert np.array_equal(got, ref), "%s: %d bytes differ" % (name, int((got != ref).sum()))
        ran += 1
    assert ran >= 7


def test_the_defaults_are_the_null_parameters(dev):
    ref, _ = sk.checker(8)
    assert np.array_equal(run_device(dev, 8, None), ref) and np.array_equal(run_device(dev, 8, {}), ref)


def test_a_plane_4_bytes_past_a_16_byte_boundary(dev):
    for name in ("dim33_el30_wide_disc", "dim3_offaxis_sdef_alt0", "dim64_el-3_sdef_alt0"):
        _, dim, params = {c[0]: c for c in sk.corpus()}[name]
        ref, _ = sk.expected(name)
        assert np.array_equal(run_device(dev, dim, params, misalign=4), ref), name
        assert np.array_equal(run_device(dev, dim, params, misalign=12), ref), name


@pytest.mark.parametrize("name", ["dim8_el5_sdef_alt50", "dim33_el30_wide_disc"])
def test_face_ranges_stitch_to_the_whole_cube(dev, name):
    _, dim, params = {c[0]: c for c in sk.corpus()}[name]
    whole, _ = sk.expected(name)
    for k in range(7):
        stitched = np.full(whole.shape, sk.GUARD, np.uint8)
        for face0, faces in ((0, k), (k, 6 - k)):
            got = run_device(dev, dim, params, face0, faces, misalign=4 * (k % 2))
            assert (got[:face0] == sk.GUARD).all() and (got[face0 + faces:] == sk.GUARD).all(), "a face outside the range was written"
            stitched[face0:face0 + faces] = got[face0:face0 + faces]
        assert np.array_equal(stitched, whole), (name, k)


def test_refusals_with_a_context_write_nothing(dev):
    from test_sky_host import refusal_cases
    lib, ctx, torch = dev
    planes = DevicePlanes(dev)
    cube = planes.blank("cube", (6, 8, 8, 4))
    base = cube.data_ptr()
    n = 0
    for kw, word in refusal_cases(lib.SkyParams):
        a = dict(cube=base, dim=8, face0=0, faces=6, params=None)
        a.update(kw)
        if a["cube"] is not None and a["cube"] != base:
            a["cube"] = base + (a["cube"] & 3)              # the misaligned addresses of the CPU tier, inside the plane
        rc = lib.lib.crychic_render_sky(ctx.handle, None if a["cube"] is None else C.c_void_p(a["cube"]), a["dim"], a["face0"], a["faces"],
                                        None if a["params"] is None else C.byref(a["params"]), None)
        assert rc == -1 and word in lib.lib.crychic_last_error().decode(), (kw, rc)
        n += 1
    assert n >= 50
    torch.cuda.synchronize()
    assert bool((cube == sk.GUARD).all()), "a refused call wrote"
    planes.verify()
    # faces == 0 is valid and writes nothing
    for face0 in (0, 3, 6):
        lib.check(lib.lib.crychic_render_sky(ctx.handle, C.c_void_p(base), 8, face0, 0, None, None))
    torch.cuda.synchronize()
    assert bool((cube == sk.GUARD).all())


def test_the_call_replays_from_a_graph(dev):
    lib, ctx, torch = dev
    name = "dim33_el5_wide_disc"
    _, dim, params = {c[0]: c for c in sk.corpus()}[name]
    ref, _ = sk.expected(name)
    planes = DevicePlanes(dev)
    cube = planes.blank("cube", (6, dim, dim, 4))
    p = sky_params(lib, params)

    def call():
        s = torch.cuda.current_stream(ctx.device)
        lib.check(lib.lib.crychic_render_sky(ctx.handle, C.c_void_p(cube.data_ptr()), dim, 0, 6, C.byref(p), C.c_void_p(s.cuda_stream)))
    call()                                  # before the capture: the code object loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        cube.fill_(sk.GUARD)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(cube.cpu().numpy().reshape(ref.shape), ref)
    planes.verify()


# ---- Crychic.render_sky, sky_sun_colour, followSun ---------------------------------------------------------------------------------

W, H, SD, CUBE = 128, 96, 256, 32


def make_app(dev):
    """A Crychic over the 128 x 96 synthetic scene with a pass-constants block of its own."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=CUBE, device="cuda:0")
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
    app.load_scene(planes)
    app.mMainPassCB = lib.PassConstants.from_buffer_copy(planes["consts"].pass_cb)
    app.blurCount, app.numDirLights, app.flags = 3, 3, LIGHT_SKY
    return app, planes


def sun_of(app):
    """The direction towards the sun of Lights[0], as the float32 values followSun hands the sky."""
    return tuple(float(np.float32(-v)) for v in app.mMainPassCB.Lights[0].Direction)


def test_render_sky_builds_the_chain(dev):
    lib, ctx, torch = dev
    from crychic_renderer_amd import CrychicError, SkyParams, geometry as g
    app, _ = make_app(dev)
    p = SkyParams.default(sunDir=sk.sun_at(12, 40), altitude=1.5)
    want, _ = sk.checker(32, dict(sunDir=sk.sun_at(12, 40), altitude=1.5))
    chain, dim, levels = app.render_sky(p, dim=32, levels=6)
    torch.cuda.synchronize()
    got = chain.cpu().numpy()
    assert (dim, levels) == (32, 6) and got.size == g.cube_chain_bytes(32, 6) and app.skyRenders == 1
    assert np.array_equal(got[:want.size].reshape(want.shape), want), "level 0 is not the checker's sky"
    flat, n = g.cube_mip_chain(want, 6)
    assert n == 6 and np.array_equal(got, flat), "the further levels are not the box chain of level 0"
    # the defaults, one level, into a tensor of the caller's
    out = torch.full((g.cube_chain_bytes(8, 1) + 16,), sk.GUARD, dtype=torch.uint8, device=ctx.device)
    chain, dim, levels = app.render_sky(dim=8, levels=1, out=out)
    torch.cuda.synchronize()
    assert chain is out and (dim, levels) == (8, 1)
    assert np.array_equal(out.cpu().numpy()[:-16].reshape(6, 8, 8, 4), sk.checker(8)[0]) and bool((out[-16:] == sk.GUARD).all())
    # what capture_environment refuses
    for kw in (dict(env_brdf=True), dict(dim=1), dict(dim=8193), dict(dim=32, levels=7), dict(dim=32, levels=0), dict(dim=32, levels=1, prefilter=True, env_brdf=True),
               dict(dim=8, levels=1, out=out[:100]), dict(dim=CUBE, levels=1, out=app.mCubeMap.view(-1))):
        with pytest.raises(CrychicError):
            app.render_sky(**kw)


def test_render_sky_with_irradiance_and_prefilter(dev):
    """irradiance=True leaves the env_sh checker's projection of level 0 in the tail, without and with prefilter=True; with env_brdf
    the chain binds and lights a frame."""
    import env_sh_lib
    lib, ctx, torch = dev
    from crychic_renderer_amd import SkyParams, geometry as g
    es = env_sh_lib.load()
    app, _ = make_app(dev)
    params = dict(sunDir=sk.sun_at(20, -30))
    want, _ = sk.checker(32, params)
    coeffs = es.project(want)
    for pre in (False, True):
        chain, dim, levels = app.render_sky(SkyParams.default(**params), dim=32, prefilter=pre, irradiance=True)
        torch.cuda.synchronize()
        got = chain.cpu().numpy()
        assert (dim, levels) == (32, 6) and got.size == g.cube_chain_sh_bytes(32, 6)
        assert np.array_equal(got[:want.size].reshape(want.shape), want), pre
        off = g.cube_sh_offset(32, 6)
        assert np.array_equal(got[off:off + 144].view(np.uint32), coeffs.reshape(-1).view(np.uint32)), pre
    chain, dim, levels = app.render_sky(SkyParams.default(**params), dim=32, prefilter=True, irradiance=True, env_brdf=True)
    assert chain.numel() == g.cube_chain_env_bytes(32, 6)
    app.Draw()
    torch.cuda.synchronize()
    before = app.mBackBuffer.cpu().numpy().copy()
    app.set_cube_map(chain, dim, levels, gloss=True, ambient_sh=True, env_brdf=True)
    app.Draw()
    torch.cuda.synchronize()
    assert (app.mBackBuffer.cpu().numpy() != before).any()


def test_follow_sun(dev):
    lib, ctx, torch = dev
    from crychic_renderer_amd import CrychicError, SkyParams
    auto, planes = make_app(dev)
    hand, _ = make_app(dev)
    plain, _ = make_app(dev)
    # unset: the frame and the bound cube are today's
    plain.Draw()
    torch.cuda.synchronize()
    frame0 = plain.mBackBuffer.cpu().numpy().copy()
    cube0 = planes["cube"].cpu().numpy().copy()
    auto.followSun = None
    auto.Draw()
    torch.cuda.synchronize()
    assert auto.followSun is None and auto.skyRenders == 0 and auto.mCubeMap is planes["cube"]
    assert np.array_equal(auto.mBackBuffer.cpu().numpy(), frame0) and np.array_equal(auto.mCubeMap.cpu().numpy(), cube0)
    # set: Draw equals render_sky + set_cube_map by hand
    auto.followSun = True
    auto.Draw()
    chain, dim, levels = hand.render_sky(SkyParams.default(sunDir=sun_of(hand)), dim=CUBE, levels=1)
    hand.set_cube_map(chain, dim, levels)
    hand.Draw()
    torch.cuda.synchronize()
    assert auto.skyRenders == 1 and auto.mCubeMap is not planes["cube"]
    want, _ = sk.checker(CUBE, dict(sunDir=sun_of(auto)))
    bound = auto.mCubeMap.cpu().numpy()[:want.size].reshape(want.shape)
    assert np.array_equal(bound, want), "the bound cube is not the checker's sky under Lights[0]"
    frame1 = auto.mBackBuffer.cpu().numpy().copy()
    assert np.array_equal(frame1, hand.mBackBuffer.cpu().numpy()) and (frame1 != frame0).any()
    assert np.array_equal(planes["cube"].cpu().numpy(), cube0), "the scene's own cube map was written"
    # the light turns: the sky is rendered anew
    low = sk.sun_at(4, 25)
    auto.mMainPassCB.Lights[0].Direction[:] = [-c for c in low]
    auto.Draw()
    torch.cuda.synchronize()
    want2, _ = sk.checker(CUBE, dict(sunDir=sun_of(auto)))
    bound2 = auto.mCubeMap.cpu().numpy()[:want.size].reshape(want.shape).copy()
    assert auto.skyRenders == 2 and (bound2 != bound).any() and np.array_equal(bound2, want2)
    frame2 = auto.mBackBuffer.cpu().numpy().copy()
    # nothing changed: no sky launch, the same cube, the same frame
    auto.Draw()
    torch.cuda.synchronize()
    assert auto.skyRenders == 2 and np.array_equal(auto.mCubeMap.cpu().numpy()[:want.size].reshape(want.shape), bound2)
    assert np.array_equal(auto.mBackBuffer.cpu().numpy(), frame2)
    # a strip draws the same deterministic cube; parameters of the caller's reach the sky and re-render it
    auto.followSun = SkyParams.default(viewSteps=5, sunSteps=3, exposure=1.0)
    auto.Draw(row0=0, rows=48)
    torch.cuda.synchronize()
    want3, _ = sk.checker(CUBE, dict(sunDir=sun_of(auto), viewSteps=5, sunSteps=3, exposure=1.0))
    assert auto.skyRenders == 3 and np.array_equal(auto.mCubeMap.cpu().numpy()[:want.size].reshape(want.shape), want3)
    with pytest.raises(CrychicError):
        auto.followSun = 3
    # the flags of the last set_cube_map are kept: a chain is rendered as a chain
    chain, dim, levels = hand.render_sky(SkyParams.default(sunDir=sun_of(hand)), dim=CUBE, prefilter=True, irradiance=True)
    hand.set_cube_map(chain, dim, levels, gloss=True, ambient_sh=True)
    hand.Draw()
    auto.followSun = True
    auto.mMainPassCB.Lights[0].Direction[:] = hand.mMainPassCB.Lights[0].Direction[:]
    auto.set_cube_map(chain.clone(), dim, levels, gloss=True, ambient_sh=True)
    auto.mCubeMap.zero_()
    auto.Draw()
    torch.cuda.synchronize()
    assert auto.skyRenders == 4 and (auto.mCubeMapLevels, auto.mCubeMapGloss, auto.mCubeMapAmbientSH) == (levels, True, True)
    from crychic_renderer_amd import geometry as g
    mine, theirs, n, off = auto.mCubeMap.cpu().numpy(), chain.cpu().numpy(), g.cube_chain_bytes(dim, levels), g.cube_sh_offset(dim, levels)
    assert np.array_equal(mine[:n], theirs[:n]) and np.array_equal(mine[off:off + 144], theirs[off:off + 144])      # the chain, the coefficients
    assert np.array_equal(auto.mBackBuffer.cpu().numpy(), hand.mBackBuffer.cpu().numpy())


def test_sky_sun_colour_is_the_host_value(dev):
    from crychic_renderer_amd import Crychic, SkyParams
    for params in (dict(), dict(sunDir=sk.sun_at(3)), dict(sunDir=sk.sun_at(-30)), dict(sunDir=(0.3, 0.5, -0.8), altitude=50.0, sunSteps=32)):
        got = np.array(Crychic.sky_sun_colour(SkyParams.default(**params)), np.float32)
        assert np.array_equal(got.view(np.uint32), sk.sun_colour(params).view(np.uint32)), params
    assert Crychic.sky_sun_colour() == Crychic.sky_sun_colour(SkyParams.default())
