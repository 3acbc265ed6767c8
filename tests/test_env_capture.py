"""Environment capture (include/crychic_hip.h "environment capture"): the six face cameras, the device-built
mip chain (crychic_generate_cube_mips == geometry.cube_mip_chain byte for byte) and Crychic.capture_environment, whose faces are
the frames of the face cameras -- checked against the CPU oracle's pipeline bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib

DIMS = (2, 6, 16, 64, 250)
POSITIONS = ((0.0, 0.0, 0.0), (1.5, 2.25, -3.0), (17.3, -4.1, 9.7))
FACE_TABLE = (((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, -1)),
              ((0, -1, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0)))


def _cameras(built_lib, pos, z_near=0.5, z_far=100.0):
    cams = (built_lib.Camera * 6)()
    assert built_lib.lib.crychic_cube_capture_cameras((C.c_float * 3)(*pos), z_near, z_far, cams) == 0
    return cams


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------

def test_capture_cameras_match_the_table(built_lib):
    pos = (1.5, 2.25, -3.0)
    cams = _cameras(built_lib, pos, 0.25, 80.0)
    half_pi = np.float32(math.pi / 2)
    for f, (look, up) in enumerate(FACE_TABLE):
        c = cams[f]
        assert tuple(c.pos) == pos and tuple(c.look) == look and tuple(c.up) == up, f
        assert np.float32(c.fovY).tobytes() == half_pi.tobytes() and c.aspect == 1.0 and c.nearZ == 0.25 and c.farZ == 80.0
    lib = built_lib.lib
    p = (C.c_float * 3)(*pos)
    assert lib.crychic_cube_capture_cameras(None, 0.5, 100.0, cams) == -1
    assert lib.crychic_cube_capture_cameras(p, 0.5, 100.0, None) == -1
    assert lib.crychic_cube_capture_cameras(p, 0.0, 100.0, cams) == -1
    assert lib.crychic_cube_capture_cameras(p, 2.0, 1.0, cams) == -1


def _sky_frame(built_lib, oracle, cam, dim, cube):
    """The oracle's frame for `cam` at dim x dim over an all-clear depth plane, sky on."""
    pcb = built_lib.PassConstants()
    st = np.zeros((4, 4, 4), np.float32)
    dirs = np.zeros((3, 3), np.float32)
    assert built_lib.lib.crychic_update_main_pass_cb(C.byref(cam), dim, dim, st.ctypes.data, dirs.ctypes.data, C.byref(pcb)) == 0
    g = np.zeros((dim, dim, 4), np.float32)
    depth = np.full((dim, dim), 0xFFFFFF, np.uint32)
    shadow = np.full((4, 2, 2), 0xFFFFFF, np.uint32)
    return oracle.deferred_light(oracle_lib.as_oracle_cb(pcb, oracle_lib.OrPassConstants), g, g, g, depth, None, shadow, cube, 1, 0.0, sky=True)


@pytest.mark.parametrize("dim", DIMS)
def test_known_answer_face_frames_are_the_cube_faces(built_lib, oracle, dim):
    """The feature's known answer: the sky frame of face camera f over a one-level cube map of the frame's own dim is face f, all four
    channels, zero differing bytes -- for the product's cameras through the product's constant builder."""
    cube = np.random.default_rng(dim).integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)
    for pos in POSITIONS:
        cams = _cameras(built_lib, pos)
        for f in range(6):
            got = _sky_frame(built_lib, oracle, cams[f], dim, cube)
            assert int((got != cube[f]).sum()) == 0, (pos, f)


def test_known_answer_detects_a_wrong_face_convention(built_lib, oracle):
    """A changed up vector, a mirrored axis or two swapped faces each break the known answer."""
    dim = 16
    cube = np.random.default_rng(7).integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)
    cams = _cameras(built_lib, POSITIONS[1])
    up = built_lib.Camera.from_buffer_copy(cams[2])
    up.up[:] = (0.0, 0.0, 1.0)
    assert not np.array_equal(_sky_frame(built_lib, oracle, up, dim, cube), cube[2])
    mirrored = built_lib.Camera.from_buffer_copy(cams[0])
    mirrored.look[:] = (-1.0, 0.0, 0.0)
    assert not np.array_equal(_sky_frame(built_lib, oracle, mirrored, dim, cube), cube[0])
    assert not np.array_equal(_sky_frame(built_lib, oracle, cams[4], dim, cube), cube[5])      # +Z and -Z swapped


def test_cube_chain_bytes(built_lib):
    lib = built_lib.lib
    for dim in (1, 5, 256, 16384):
        full = int(dim).bit_length()
        for levels in (1, 2, full):
            assert lib.crychic_cube_chain_bytes(dim, levels) == sum(6 * 4 * max(dim >> k, 1) ** 2 for k in range(levels)), (dim, levels)
    assert lib.crychic_cube_chain_bytes(256, 0) == 0
    assert lib.crychic_cube_chain_bytes(4, 40) == 24 * (16 + 4 + 1) + 24 * 37       # levels past 1 x 1 count 24 bytes each


def test_generate_cube_mips_refuses_a_null_context(built_lib):
    assert built_lib.lib.crychic_generate_cube_mips(None, None, 16, 2, None) == -1


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(built_lib):
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


def _noise_cube(dim, seed=None):
    return np.random.default_rng(dim if seed is None else seed).integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)


def _device_mips(ctx, cube, levels, guard=0):
    """crychic_generate_cube_mips over level 0 = `cube` in a buffer pre-filled with 0xA5 (`guard` bytes past the chain)."""
    import torch
    from crychic_renderer_amd import lib
    from crychic_renderer_amd._lib import check
    dim = cube.shape[1]
    n = int(lib.crychic_cube_chain_bytes(dim, levels))
    buf = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=ctx.device)
    buf[:cube.size] = torch.from_numpy(cube.reshape(-1)).to(ctx.device)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(ctx.device)
    check(lib.crychic_generate_cube_mips(ctx.handle, C.c_void_p(buf.data_ptr()), dim, levels, C.c_void_p(s.cuda_stream)))
    s.synchronize()
    return buf.cpu().numpy(), n


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 3, 5, 64, 65, 96, 130, 200, 256])
def test_mips_equal_the_definition(ctx, dim):
    """dims 65, 96 and 130: level 0 is no multiple of the tile and the second level is odd; 256 takes two launches."""
    from crychic_renderer_amd import geometry as g
    cube = _noise_cube(dim)
    ref, levels = g.cube_mip_chain(cube)
    assert levels == int(dim).bit_length()
    got, n = _device_mips(ctx, cube, levels, guard=64)
    assert n == ref.size and np.array_equal(got[:n], ref)
    assert (got[n:] == 0xA5).all()


@pytest.mark.gpu
def test_mips_leave_the_rest_alone(ctx):
    from crychic_renderer_amd import geometry as g
    cube = _noise_cube(256, 1)
    ref, levels = g.cube_mip_chain(cube, 3)
    got, n = _device_mips(ctx, cube, 3, guard=6 * 4 * 32 * 32 + 4096)       # the guard covers where level 3 would go
    assert levels == 3 and n == ref.size
    assert np.array_equal(got[:cube.size], cube.reshape(-1))                # level 0 unchanged
    assert np.array_equal(got[:n], ref)
    assert (got[n:] == 0xA5).all()
    one, n1 = _device_mips(ctx, cube, 1, guard=4096)                        # levels == 1: a no-op that succeeds
    assert np.array_equal(one[:n1], cube.reshape(-1)) and (one[n1:] == 0xA5).all()


@pytest.mark.gpu
def test_mips_argument_errors(ctx):
    import torch
    from crychic_renderer_amd import lib
    buf = torch.zeros((int(lib.crychic_cube_chain_bytes(16, 5)),), dtype=torch.uint8, device=ctx.device)
    s = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    p = C.c_void_p(buf.data_ptr())
    assert lib.crychic_generate_cube_mips(ctx.handle, None, 16, 5, s) == -1
    assert lib.crychic_generate_cube_mips(ctx.handle, p, 0, 1, s) == -1
    assert lib.crychic_generate_cube_mips(ctx.handle, p, 16, 0, s) == -1
    assert lib.crychic_generate_cube_mips(ctx.handle, p, 16, 6, s) == -1
    assert b"6 cube map levels, a 16-texel face has at most 5" in lib.crychic_last_error()
    assert lib.crychic_generate_cube_mips(ctx.handle, p, 16, 5, s) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_mips_run_on_the_callers_stream(ctx):
    """Level 0 reaches the buffer on a side stream behind a few milliseconds of other work, and the chain is built on that stream: a
    launch on any other stream would start at once and reduce the 0xA5 fill instead of level 0."""
    import torch
    from crychic_renderer_amd import geometry as g, lib
    from crychic_renderer_amd._lib import check
    cube = _noise_cube(96, 2)
    ref, levels = g.cube_mip_chain(cube)
    n = int(lib.crychic_cube_chain_bytes(96, levels))
    buf = torch.full((n,), 0xA5, dtype=torch.uint8, device=ctx.device)
    level0 = torch.from_numpy(cube.reshape(-1)).to(ctx.device)
    ballast = torch.empty((1 << 28,), dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=ctx.device)
    with torch.cuda.stream(side):
        for k in range(16):
            ballast.fill_(k)
        buf[:cube.size].copy_(level0)
    check(lib.crychic_generate_cube_mips(ctx.handle, C.c_void_p(buf.data_ptr()), 96, levels, C.c_void_p(side.cuda_stream)))
    side.synchronize()
    assert np.array_equal(buf.cpu().numpy(), ref)


# The capture scene: the box-and-grid scene with the reference materials and procedural textures, the probe above the grid among
# the boxes (box centres are multiples of 5 in x and z, 1.6 units high), 64-texel faces, 256-texel cascades, blurCount 2.
DIM, SD, BC, SRC_DIM = 64, 256, 2, 32
PROBE = (2.5, 1.25, 2.5)


class _Scene:
    def __init__(self, ctx):
        import torch
        from crychic_renderer_amd import SceneGeometry, geometry as g, scene
        self.items, self.shadow_items = g.cascade_scene_items(), g.cascade_scene_items(shadow_layer=True)
        self.materials, self.textures = g.reference_materials(), g.procedural_textures(16)
        self.geo = SceneGeometry(ctx, self.items, self.materials, self.textures)
        self.shadow_geo = SceneGeometry(ctx, self.shadow_items)
        self.consts = scene.Constants(DIM, DIM, SD)                       # the main frame: default camera, reference lights
        self.source = _noise_cube(SRC_DIM, 11)
        self.source_chain, self.source_levels = g.cube_mip_chain(self.source)
        self.source_dev = torch.from_numpy(self.source).to(ctx.device)
        self.source_chain_dev = torch.from_numpy(self.source_chain).to(ctx.device)
        self.randvec = torch.from_numpy(self.consts.randvec.copy()).to(ctx.device)
        self.cams = g.cube_capture_cameras(PROBE)

    def app(self, ctx, chain=False):
        from crychic_renderer_amd import Crychic
        a = Crychic(ctx, DIM, DIM, self.randvec, self.source_dev, shadow_dim=SD)
        a.mMainPassCB, a.mSsaoCB = self.consts.pass_cb, self.consts.ssao_cb
        a.blurCount, a.numDirLights = BC, 1
        if chain:
            a.set_cube_map(self.source_chain_dev, SRC_DIM, self.source_levels)
        return a


@pytest.fixture(scope="module")
def cap(ctx):
    return _Scene(ctx)


@pytest.fixture(scope="module")
def face_planes(cap, oracle, built_lib):
    """The CPU oracle's pipeline for each face camera, lit with the one-level source: cascades, normals, depth, G-buffer, SSAO."""
    import raster_util
    from crychic_renderer_amd import scene
    pcf = built_lib.lib.crychic_pcf_search_radius(SD, 1)
    out = []
    for f in range(6):
        consts = scene.Constants(DIM, DIM, SD, cam=cap.cams[f])
        fr = raster_util.oracle_frame(oracle, consts, cap.items, cap.shadow_items, cap.materials, cap.textures, DIM, DIM, SD, cap.source,
                                      BC, 1, pcf, sky=True)
        fr["pcb"] = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
        out.append(fr)
    return out


def _faces(chain, dim):
    return chain[:6 * dim * dim * 4].cpu().numpy().reshape(6, dim, dim, 4)


@pytest.mark.gpu
def test_sky_only_capture_is_the_source(ctx, cap):
    import torch
    from crychic_renderer_amd import Crychic, geometry as g
    src = _noise_cube(64, 5)
    app = Crychic(ctx, 128, 96, cap.randvec, torch.from_numpy(src).to(ctx.device), shadow_dim=SD)
    app.mMainPassCB, app.mSsaoCB = cap.consts.pass_cb, cap.consts.ssao_cb
    chain, dim, levels = app.capture_environment((1.5, 2.25, -3.0), None, dim=64, shadow_dim=SD)
    torch.cuda.synchronize()
    assert (dim, levels) == (64, 7)
    ref, n = g.cube_mip_chain(src)
    assert n == 7 and np.array_equal(_faces(chain, 64), src)
    assert np.array_equal(chain.cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("source_chain", [False, True])
def test_captured_faces_are_the_oracle_frames(ctx, cap, face_planes, oracle, built_lib, source_chain):
    import torch
    app = cap.app(ctx, chain=source_chain)
    chain, dim, levels = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=DIM, shadow_dim=SD)
    torch.cuda.synchronize()
    got = _faces(chain, DIM)
    pcf = built_lib.lib.crychic_pcf_search_radius(SD, 1)
    covered = 0
    for f, fr in enumerate(face_planes):
        ref = fr["rgba8"]
        if source_chain:
            ref = oracle.deferred_light(fr["pcb"], fr["g0"], fr["g1"], fr["g2"], fr["depth"], fr["ao"], fr["shadow"], cap.source_chain, 1, pcf,
                                        sky=True, cube_dim=SRC_DIM, cube_levels=cap.source_levels)
        assert int((got[f] != ref).sum()) == 0, f
        covered += int((fr["depth"] < 0xFFFFFF).sum())
    assert covered > DIM * DIM                        # the faces do see the scene: more than one face's worth of covered pixels
    from crychic_renderer_amd import geometry as g
    assert np.array_equal(chain.cpu().numpy(), g.cube_mip_chain(got)[0])


@pytest.mark.gpu
def test_captured_faces_with_local_lights_are_draws_frames(ctx, cap):
    """One point light and one shadowed spot light: each face equals the frame Crychic.Draw produces for that camera."""
    import torch
    import raster_util
    from crychic_renderer_amd import Crychic, LIGHT_SKY, PassConstants, scene

    def lights(a):
        a.set_point_lights(scene.shadow_point_lights(1))
        a.set_spot_lights(scene.shadow_spot_lights(1))
        a.set_spot_shadows(1, dim=128, geometry=cap.shadow_geo)

    app = cap.app(ctx)
    lights(app)
    chain, _, _ = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=DIM, shadow_dim=SD)
    plain, _, _ = cap.app(ctx).capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=DIM, shadow_dim=SD, levels=1)
    torch.cuda.synchronize()
    got = _faces(chain, DIM)
    assert not np.array_equal(got, _faces(plain, DIM))                    # the local lights reach the probe's surroundings
    ref_app = Crychic(ctx, DIM, DIM, cap.randvec, cap.source_dev, shadow_dim=SD)
    ref_app.blurCount, ref_app.numDirLights, ref_app.flags = BC, 1, LIGHT_SKY
    lights(ref_app)
    for f in range(6):
        consts = scene.Constants(DIM, DIM, SD, cam=cap.cams[f])
        ref_app.mMainPassCB, ref_app.mSsaoCB = consts.pass_cb, consts.ssao_cb
        cbs = []
        for k in range(4):
            cb = PassConstants()
            cb.ViewProj[:] = list(raster_util.light_viewproj_t(consts, k))
            cbs.append(cb)
        cap.shadow_geo.DrawSceneToShadowMaps(cbs, [ref_app.mShadowMap.Resource(k) for k in range(4)])
        cap.geo.DrawNormalsDepthAndGBuffer(consts.pass_cb, ref_app.mSsao.mNormalMap, ref_app.mDeferred.mGBuffer, ref_app.mDepthStencilBuffer)
        ref_app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(got[f], ref_app.mBackBuffer.cpu().numpy()), f


@pytest.mark.gpu
def test_capture_refuses_aliasing_and_odd_sizes(ctx, cap):
    import torch
    from crychic_renderer_amd import CrychicError
    app = cap.app(ctx)
    bound = app.mCubeMap
    before = bound.cpu().numpy().copy()
    with pytest.raises(CrychicError) as e:
        app.capture_environment(PROBE, None, dim=16, levels=1, shadow_dim=SD, out=bound.view(-1))
    assert e.value.status == -1 and "aliases" in str(e.value)
    with pytest.raises(CrychicError) as e:
        app.capture_environment(PROBE, None, dim=63, shadow_dim=SD)
    assert e.value.status == -1 and "even" in str(e.value)          # refused as every odd frame size is
    with pytest.raises(CrychicError):
        app.capture_environment(PROBE, None, dim=0, shadow_dim=SD)
    with pytest.raises(CrychicError):
        app.capture_environment(PROBE, None, dim=16, levels=6, shadow_dim=SD)
    chain, dim, levels = app.capture_environment(PROBE, None, dim=16, shadow_dim=SD)
    torch.cuda.synchronize()
    assert app.mCubeMap is bound and app.mCubeMapLevels == 1 and np.array_equal(bound.cpu().numpy(), before)
    again, _, _ = app.capture_environment(PROBE, None, dim=16, shadow_dim=SD, out=chain)       # re-capture into the same buffer
    assert again.data_ptr() == chain.data_ptr()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_the_reflection_uses_the_captured_chain(ctx, cap, oracle, built_lib):
    """The captured chain bound with set_cube_map: the main frame equals the oracle's frame lit with that chain, and differs from the
    frame lit with the source -- the probe bites."""
    import torch
    import raster_util
    from crychic_renderer_amd import LIGHT_SKY
    app = cap.app(ctx)
    chain, dim, levels = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=DIM, shadow_dim=SD)
    app.set_cube_map(chain, dim, levels)
    app.flags = LIGHT_SKY
    cbs = []
    for k in range(4):
        cb = built_lib.PassConstants()
        cb.ViewProj[:] = list(raster_util.light_viewproj_t(cap.consts, k))
        cbs.append(cb)
    cap.shadow_geo.DrawSceneToShadowMaps(cbs, [app.mShadowMap.Resource(k) for k in range(4)])
    cap.geo.DrawNormalsDepthAndGBuffer(cap.consts.pass_cb, app.mSsao.mNormalMap, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    app.Draw()
    torch.cuda.synchronize()
    got = app.mBackBuffer.cpu().numpy()
    pcf = built_lib.lib.crychic_pcf_search_radius(SD, 1)
    fr = raster_util.oracle_frame(oracle, cap.consts, cap.items, cap.shadow_items, cap.materials, cap.textures, DIM, DIM, SD,
                                  chain.cpu().numpy(), BC, 1, pcf, sky=True, cube_dim=dim, cube_levels=levels)
    assert np.array_equal(got, fr["rgba8"])
    pcb = oracle_lib.as_oracle_cb(cap.consts.pass_cb, oracle_lib.OrPassConstants)
    with_source = oracle.deferred_light(pcb, fr["g0"], fr["g1"], fr["g2"], fr["depth"], fr["ao"], fr["shadow"], cap.source, 1, pcf, sky=True)
    assert not np.array_equal(got, with_source)
