"""The C++ veneer's ambient light from the environment (include/crychic/CRYCHIC.h SetEnvironmentAmbient): tests/cpp/env_ambient_driver.cpp
captures the built-in scene through the veneer with the irradiance projection on and renders a frame with the chain and its tail bound;
the tail and the frame are compared with the Python path's (capture_environment(irradiance=True), set_cube_map(ambient_sh=True)) bit
for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest


def test_env_ambient_driver_compiles(built_lib):
    """CPU tier: the veneer with SetEnvironmentAmbient compiles and links against libcrychic_hip.so."""
    import test_cpp_veneer
    assert os.path.exists(test_cpp_veneer.build_driver("env_ambient_driver"))


@pytest.mark.gpu
@pytest.mark.parametrize("gloss", [0, 1])
def test_veneer_env_ambient_equals_the_python_path(built_lib, tmp_path, gloss):
    import env_sh_lib
    import raster_util
    import test_cpp_veneer
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, PassConstants, SceneGeometry, geometry as g, scene
    W, H, SD, CD, BC, DIM, CAP_SD = 64, 64, 256, 32, 2, 32, 256
    pos = (2.5, 1.25, 2.5)
    d = str(tmp_path)
    exe = test_cpp_veneer.build_driver("env_ambient_driver")
    source = np.random.default_rng(11).integers(0, 256, (6, CD, CD, 4), dtype=np.uint8)
    source.tofile(d + "/cube.bin")
    r = subprocess.run([exe, d] + [str(v) for v in (W, H, SD, CD, BC, DIM, CAP_SD) + pos + (gloss,)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want_levels = 6 if gloss else 1
    assert "env ambient driver ok dim 32 levels %d" % want_levels in r.stdout
    chain = np.fromfile(d + "/chain.bin", dtype=np.uint8)
    out = np.fromfile(d + "/out.bin", dtype=np.uint8).reshape(H, W, 4)

    ctx = Context(0)
    consts = scene.Constants(W, H, SD)
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials())
    shadow_geo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), torch.from_numpy(source).to(ctx.device), shadow_dim=SD)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    app.blurCount, app.numDirLights, app.flags = BC, 1, LIGHT_SKY
    got, dim, levels = app.capture_environment(pos, geo, shadow_geo, dim=DIM, shadow_dim=CAP_SD, levels=want_levels, prefilter=bool(gloss),
                                               irradiance=True)
    torch.cuda.synchronize()
    assert (dim, levels) == (DIM, want_levels)
    mine = got.cpu().numpy()
    off, n = g.cube_sh_offset(dim, levels), g.cube_chain_bytes(dim, levels)
    assert chain.size == mine.size == g.cube_chain_sh_bytes(dim, levels)
    # the cube map, the coefficient block and the accumulators; the padding and the tail's reserved bytes are nobody's
    assert np.array_equal(chain[:n], mine[:n]) and np.array_equal(chain[off:off + 368], mine[off:off + 368])
    level0 = chain[:6 * dim * dim * 4].reshape(6, dim, dim, 4)
    block = chain[off:off + 144].view(np.float32).reshape(9, 4)
    assert np.array_equal(block.view(np.uint32), env_sh_lib.load().project(level0).view(np.uint32))
    # the frame with the chain bound and the flag set: the veneer's own constants drive the Python path
    app.set_cube_map(got, dim, levels, gloss=bool(gloss), ambient_sh=True)
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
    lit = app.mBackBuffer.cpu().numpy().copy()
    assert np.array_equal(out, lit)
    app.set_cube_map(got, dim, levels, gloss=bool(gloss))          # the constant ambient term over the same cube map is another frame
    app.Draw()
    torch.cuda.synchronize()
    assert (app.mBackBuffer.cpu().numpy() != lit).any()
    ctx.close()
