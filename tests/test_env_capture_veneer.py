"""The C++ veneer's environment capture (include/crychic/CRYCHIC.h CaptureEnvironment): tests/cpp/env_capture_driver.cpp captures the
built-in scene through the veneer, and its chain and the frame rendered with it are compared with the Python path's bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest


def test_env_capture_driver_compiles(built_lib):
    """CPU tier: the veneer with CaptureEnvironment compiles and links against libcrychic_hip.so."""
    import test_cpp_veneer
    assert os.path.exists(test_cpp_veneer.build_driver("env_capture_driver"))


@pytest.mark.gpu
@pytest.mark.parametrize("local_lights", [False, True])
def test_veneer_capture_equals_the_python_capture(built_lib, tmp_path, local_lights):
    """local_lights: one point light and one shadowed spot light on the veneer object, which its probe reads in place."""
    import raster_util
    import test_cpp_veneer
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, PassConstants, SceneGeometry, geometry as g, scene
    W, H, SD, CD, BC, DIM, CAP_SD = 64, 64, 256, 32, 2, 64, 256
    pos = (2.5, 1.25, 2.5)
    d = str(tmp_path)
    exe = test_cpp_veneer.build_driver("env_capture_driver")
    source = np.random.default_rng(11).integers(0, 256, (6, CD, CD, 4), dtype=np.uint8)
    source.tofile(d + "/cube.bin")
    points, spots = scene.shadow_point_lights(1), scene.shadow_spot_lights(1)
    open(d + "/points.bin", "wb").write(bytes(points))
    open(d + "/spots.bin", "wb").write(bytes(spots))
    r = subprocess.run([exe, d] + [str(v) for v in (W, H, SD, CD, BC, DIM, 0, CAP_SD) + pos] + (["lights"] if local_lights else []),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "env capture driver ok dim 64 levels 7" in r.stdout
    chain = np.fromfile(d + "/chain.bin", dtype=np.uint8)
    out = np.fromfile(d + "/out.bin", dtype=np.uint8).reshape(H, W, 4)

    ctx = Context(0)
    consts = scene.Constants(W, H, SD)
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials())
    shadow_geo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), torch.from_numpy(source).to(ctx.device), shadow_dim=SD)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    app.blurCount, app.numDirLights, app.flags = BC, 1, LIGHT_SKY
    if local_lights:
        app.set_point_lights(points)
        app.set_spot_lights(spots)
        app.set_spot_shadows(1, dim=128, geometry=shadow_geo)
    got, dim, levels = app.capture_environment(pos, geo, shadow_geo, dim=DIM, shadow_dim=CAP_SD)
    torch.cuda.synchronize()
    assert (dim, levels) == (DIM, 7)
    assert np.array_equal(chain, got.cpu().numpy())
    # the frame with the captured chain bound: the veneer's own constants drive the Python path
    app.set_cube_map(got, dim, levels)
    app.mMainPassCB, app.mSsaoCB = PassConstants(), type(consts.ssao_cb)()
    C.memmove(C.addressof(app.mMainPassCB), open(d + "/pass_cb.bin", "rb").read(), C.sizeof(app.mMainPassCB))
    C.memmove(C.addressof(app.mSsaoCB), open(d + "/ssao_cb.bin", "rb").read(), C.sizeof(app.mSsaoCB))
    cbs = []
    for k in range(4):
        cb = PassConstants()
        cb.ViewProj[:] = list(raster_util.light_viewproj_t(consts, k))
        cbs.append(cb)
    shadow_geo.DrawSceneToShadowMaps(cbs, [app.mShadowMap.Resource(k) for k in range(4)])
    geo.DrawNormalsDepthAndGBuffer(app.mMainPassCB, app.mSsao.mNormalMap, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(out, app.mBackBuffer.cpu().numpy())
    ctx.close()
