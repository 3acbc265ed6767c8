"""The C++ veneer's split-sum specular from the environment (include/crychic/CRYCHIC.h SetEnvironmentSpecular): tests/cpp/env_brdf_driver.cpp
captures the built-in scene through the veneer with glossy reflections and the environment BRDF table on and renders a frame with the
chain, its tail and the table bound; the table and the frame are compared with the Python path's (capture_environment(prefilter=True,
env_brdf=True), set_cube_map(gloss=True, env_brdf=True)) bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest


def test_env_brdf_driver_compiles(built_lib):
    """CPU tier: the veneer with SetEnvironmentSpecular compiles and links against libcrychic_hip.so."""
    import test_cpp_veneer
    assert os.path.exists(test_cpp_veneer.build_driver("env_brdf_driver"))


@pytest.mark.gpu
@pytest.mark.parametrize("ambient", [0, 1])
def test_veneer_env_specular_equals_the_python_path(built_lib, tmp_path, ambient):
    import env_brdf_lib
    import raster_util
    import test_cpp_veneer
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, PassConstants, SceneGeometry, geometry as g, scene
    W, H, SD, CD, BC, DIM, CAP_SD = 64, 64, 256, 32, 2, 32, 256
    pos = (2.5, 1.25, 2.5)
    d = str(tmp_path)
    exe = test_cpp_veneer.build_driver("env_brdf_driver")
    source = np.random.default_rng(11).integers(0, 256, (6, CD, CD, 4), dtype=np.uint8)
    source.tofile(d + "/cube.bin")
    r = subprocess.run([exe, d] + [str(v) for v in (W, H, SD, CD, BC, DIM, CAP_SD) + pos + (ambient,)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "env brdf driver ok dim 32 levels 6" in r.stdout
    chain = np.fromfile(d + "/chain.bin", dtype=np.uint8)
    out = np.fromfile(d + "/out.bin", dtype=np.uint8).reshape(H, W, 4)

    ctx = Context(0)
    consts = scene.Constants(W, H, SD)
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials())
    shadow_geo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), torch.from_numpy(source).to(ctx.device), shadow_dim=SD)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    app.blurCount, app.numDirLights, app.flags = BC, 1, LIGHT_SKY
    got, dim, levels = app.capture_environment(pos, geo, shadow_geo, dim=DIM, shadow_dim=CAP_SD, prefilter=True, irradiance=bool(ambient),
                                               env_brdf=True)
    torch.cuda.synchronize()
    assert (dim, levels) == (DIM, 6)
    mine = got.cpu().numpy()
    off, n = g.cube_env_brdf_offset(dim, levels), g.cube_chain_bytes(dim, levels)
    assert chain.size == mine.size == g.cube_chain_env_bytes(dim, levels)
    # the chain and the table (and the tail's coefficients and accumulators when it is filled); the padding is nobody's
    assert np.array_equal(chain[:n], mine[:n]) and np.array_equal(chain[off:], mine[off:])
    assert np.array_equal(chain[off:].view(np.uint32), env_brdf_lib.load().table()[0])
    if ambient:
        assert np.array_equal(chain[off - 512:off - 512 + 368], mine[off - 512:off - 512 + 368])
    # the frame with the chain bound and the flags set: the veneer's own constants drive the Python path
    app.set_cube_map(got, dim, levels, gloss=True, ambient_sh=bool(ambient), env_brdf=True)
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
    app.set_cube_map(got, dim, levels, gloss=True, ambient_sh=bool(ambient))     # the reference's weight over the same chain is another frame
    app.Draw()
    torch.cuda.synchronize()
    assert (app.mBackBuffer.cpu().numpy() != lit).any()
    ctx.close()
