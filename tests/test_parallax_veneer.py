"""The C++ veneer's parallax-corrected reflections (include/crychic/CRYCHIC.h SetReflectionProbeBox): tests/cpp/parallax_driver.cpp
captures the built-in scene through the veneer with glossy reflections, the environment BRDF table and a probe box on and renders a
frame with the chain bound; the probe volume and the frame are compared with the Python path's (capture_environment(prefilter=True,
env_brdf=True, probe_box=...), set_cube_map(gloss=True, env_brdf=True, parallax=True)) byte for byte, and clearing the box gives the
Python path's frame without the flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest


def test_parallax_driver_compiles(built_lib):
    """CPU tier: the veneer with SetReflectionProbeBox compiles and links against libcrychic_hip.so."""
    import test_cpp_veneer
    assert os.path.exists(test_cpp_veneer.build_driver("parallax_driver"))


@pytest.mark.gpu
def test_veneer_probe_box_equals_the_python_path(built_lib, tmp_path):
    import parallax_lib
    import raster_util
    import test_cpp_veneer
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, PassConstants, SceneGeometry, geometry as g, scene
    W, H, SD, CD, BC, DIM, CAP_SD = 64, 64, 256, 32, 2, 16, 256
    pos = (2.5, 1.25, 2.5)
    box = ((0.25, -0.5, 0.25), (4.75, 6.0, 4.75))
    d = str(tmp_path)
    exe = test_cpp_veneer.build_driver("parallax_driver")
    source = np.random.default_rng(11).integers(0, 256, (6, CD, CD, 4), dtype=np.uint8)
    source.tofile(d + "/cube.bin")
    r = subprocess.run([exe, d] + [str(v) for v in (W, H, SD, CD, BC, DIM, CAP_SD) + pos + box[0] + box[1]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "parallax driver ok dim 16 levels 5" in r.stdout
    chain = np.fromfile(d + "/chain.bin", dtype=np.uint8)
    out, cleared, again = (np.fromfile(d + "/" + n, dtype=np.uint8).reshape(H, W, 4) for n in ("out.bin", "out_cleared.bin", "out_again.bin"))

    ctx = Context(0)
    consts = scene.Constants(W, H, SD)
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials())
    shadow_geo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), torch.from_numpy(source).to(ctx.device), shadow_dim=SD)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    app.blurCount, app.numDirLights, app.flags = BC, 1, LIGHT_SKY
    got, dim, levels = app.capture_environment(pos, geo, shadow_geo, dim=DIM, shadow_dim=CAP_SD, prefilter=True, env_brdf=True, probe_box=box)
    torch.cuda.synchronize()
    assert (dim, levels) == (DIM, 5)
    mine = got.cpu().numpy()
    off, n, tab = g.cube_probe_offset(dim, levels), g.cube_chain_bytes(dim, levels), g.cube_env_brdf_offset(dim, levels)
    assert chain.size == mine.size == g.cube_chain_env_bytes(dim, levels)
    # the chain, the probe volume and the table; the rest of the tail and the padding are nobody's
    assert np.array_equal(chain[:n], mine[:n]) and np.array_equal(chain[tab:], mine[tab:])
    assert np.array_equal(chain[off:off + 48], mine[off:off + 48])
    assert np.array_equal(chain[off:off + 48].view(np.uint32), parallax_lib.probe_floats(pos, *box).view(np.uint32))
    # the frames with the chain bound: the veneer's own constants drive the Python path
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
    app.set_cube_map(got, dim, levels, gloss=True, env_brdf=True, parallax=True)
    app.Draw()
    torch.cuda.synchronize()
    lit = app.mBackBuffer.cpu().numpy().copy()
    assert np.array_equal(out, lit) and np.array_equal(again, lit)
    app.set_cube_map(got, dim, levels, gloss=True, env_brdf=True)        # clearing the box restores the frame without the flag
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.cpu().numpy()
    assert np.array_equal(cleared, plain) and (plain != lit).any()
    ctx.close()
