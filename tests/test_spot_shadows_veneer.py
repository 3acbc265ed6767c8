"""The C++ veneer's shadowed spot lights (include/crychic/CRYCHIC.h SetSpotShadows): tests/cpp/spot_shadow_driver.cpp renders
through CRYCHIC::Draw and its frames are compared with the Python path's (the C entries) bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import scene_util
from test_spot_lights import spots_for_test
from test_spot_shadows import random_maps


def test_spot_shadow_driver_compiles(built_lib):
    """CPU tier: the veneer with SetSpotShadows compiles and links against libcrychic_hip.so."""
    import test_cpp_veneer
    assert os.path.exists(test_cpp_veneer.build_driver("spot_shadow_driver"))


@pytest.mark.gpu
def test_veneer_set_spot_shadows(built_lib, tmp_path):
    """SetLocalLights + SetSpotShadows(3, 128), then Draw: the frame equals the Python path's (Crychic.set_spot_shadows with the
    same maps) bit for bit; SetSpotShadows(0) gives back the unshadowed frame; the argument errors throw (checked in the driver).
    The built-in scene with its producer passes: the spot map is rendered after the cascades and the shadowed frame is nowhere
    brighter than the unshadowed one, and darker somewhere."""
    import subprocess
    import torch
    import test_cpp_veneer
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, scene
    from crychic_renderer_amd._lib import PassConstants, SsaoConstants
    exe = test_cpp_veneer.build_driver("spot_shadow_driver")
    W, H, SD, CD, BC, NL, COUNT, DIM = 128, 96, 256, 32, 3, 3, 3, 128
    pl = scene_util.cpu_scene(W, H, SD, CD)
    p = scene_util.np_planes(pl)
    d = str(tmp_path)
    p["depth"].tofile(d + "/depth.bin"); p["normal"].tofile(d + "/normal.bin"); p["cube"].tofile(d + "/cube.bin")
    for i in range(3):
        p["g%d" % i].tofile(d + "/g%d.bin" % i)
    for i in range(4):
        p["shadow"][i].tofile(d + "/shadow%d.bin" % i)
    spots = spots_for_test()
    open(d + "/spots.bin", "wb").write(bytes(spots))
    open(d + "/scene_spots.bin", "wb").write(bytes(scene.shadow_spot_lights(1)))
    maps = random_maps(COUNT, DIM, 21)
    for k in range(COUNT):
        maps[k].tofile(d + "/spotmap%d.bin" % k)
    r = subprocess.run([exe, d, str(W), str(H), str(SD), str(CD), str(BC), str(NL), str(COUNT), str(DIM)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spot shadow driver ok" in r.stdout
    out = np.fromfile(d + "/out.bin", dtype=np.uint8).reshape(H, W, 4)
    out0 = np.fromfile(d + "/out_noshadow.bin", dtype=np.uint8).reshape(H, W, 4)

    ctx = Context(0)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).to(ctx.device)
           for k, v in p.items()}
    app = Crychic(ctx, W, H, dev["randvec"], dev["cube"], shadow_dim=SD)
    app.load_scene({**dev, "consts": pl["consts"]})
    app.blurCount, app.numDirLights, app.flags = BC, NL, LIGHT_SKY
    app.mMainPassCB, app.mSsaoCB = PassConstants(), SsaoConstants()
    C.memmove(C.addressof(app.mMainPassCB), open(d + "/pass_cb.bin", "rb").read(), C.sizeof(app.mMainPassCB))
    C.memmove(C.addressof(app.mSsaoCB), open(d + "/ssao_cb.bin", "rb").read(), C.sizeof(app.mSsaoCB))
    app.pcfSearchRadius = built_lib.lib.crychic_pcf_search_radius(SD, 1)
    app.set_spot_lights(spots)
    app.set_spot_shadows(COUNT, dim=DIM)
    # the veneer wrote the same transforms into the pass constants it dumped
    for k in range(COUNT):
        assert list(app._spotShadow[1][k]) == list(app.mMainPassCB.ShadowTransforms[4 + k])
    for k in range(4 + COUNT, 12):
        assert not any(app.mMainPassCB.ShadowTransforms[k])
    app.mSpotShadowMaps.copy_(torch.from_numpy(maps.view(np.int32)))
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(out, app.mBackBuffer.cpu().numpy())
    app.set_spot_shadows(0)
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(out0, app.mBackBuffer.cpu().numpy())
    assert not np.array_equal(out, out0)
    ctx.close()

    sh = np.fromfile(d + "/scene_shadowed.bin", dtype=np.uint8).reshape(H, W, 4).astype(np.int32)
    un = np.fromfile(d + "/scene_unshadowed.bin", dtype=np.uint8).reshape(H, W, 4).astype(np.int32)
    smap = np.fromfile(d + "/scene_spotmap0.bin", dtype=np.uint32)
    assert (smap < 0xFFFFFF).mean() > 0.2                                   # the light sees the box and the grid
    assert (sh <= un).all() and (sh < un).any()
