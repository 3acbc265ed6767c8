"""The C++ veneer's shadowed point lights (include/crychic/CRYCHIC.h SetPointShadows): tests/cpp/point_shadows_driver.cpp renders
through CRYCHIC::Draw and its frames are compared with the Python path's (the C entries) bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scene_util
from local_lights_util import DRIVER_FRAME, _app, _device_scene, random_maps


def test_point_shadow_driver_compiles(built_lib):
    """CPU tier: the veneer with SetPointShadows compiles and links against libcrychic_hip.so."""
    import test_cpp_veneer
    assert os.path.exists(test_cpp_veneer.build_driver("point_shadows_driver"))


@pytest.mark.gpu
def test_veneer_set_point_shadows(built_lib, tmp_path):
    """SetLocalLights + SetPointShadows(2, 64), then Draw: the frame equals the Python path's (Crychic.set_point_shadows with the
    same faces, crychic_draw_hot_path_point_shadows) bit for bit; SetPointShadows(0) gives back the unshadowed frame; the argument
    errors throw (checked in the driver).  The built-in scene with its producer passes: the faces are rendered and the shadowed
    frame is nowhere brighter than the unshadowed one, and darker somewhere."""
    import test_cpp_veneer
    import torch
    from crychic_renderer_amd import Context, scene
    from crychic_renderer_amd._lib import PassConstants, SsaoConstants
    F = DRIVER_FRAME
    W, H, SD, CD, BC, NL = F["W"], F["H"], F["SD"], F["CD"], F["BC"], F["NL"]
    COUNT, DIM = 2, 64
    d = str(tmp_path)
    exe = test_cpp_veneer.build_driver("point_shadows_driver")
    pl = scene_util.cpu_scene(W, H, SD, CD)
    p = scene_util.np_planes(pl)
    p["depth"].tofile(d + "/depth.bin"); p["normal"].tofile(d + "/normal.bin"); p["cube"].tofile(d + "/cube.bin")
    for i in range(3):
        p["g%d" % i].tofile(d + "/g%d.bin" % i)
    for i in range(4):
        p["shadow"][i].tofile(d + "/shadow%d.bin" % i)
    points = scene.shadow_point_lights(4)
    open(d + "/points.bin", "wb").write(bytes(points))
    open(d + "/scene_points.bin", "wb").write(bytes(scene.shadow_point_lights(1)))
    cubes = random_maps(COUNT * 6, DIM, 31).reshape(COUNT, 6, DIM, DIM)
    for k in range(COUNT):
        cubes[k].tofile(d + "/pointmap%d.bin" % k)
    r = subprocess.run([exe, d] + [str(v) for v in (W, H, SD, CD, BC, NL, COUNT, DIM)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "point shadows driver ok" in r.stdout
    out = np.fromfile(d + "/out_point.bin", dtype=np.uint8).reshape(H, W, 4)
    out0 = np.fromfile(d + "/out_point_none.bin", dtype=np.uint8).reshape(H, W, 4)

    ctx = Context(0)
    _, _, dev = _device_scene(ctx, W, H, SD, CD)
    app = _app(ctx, W, H, dev, pl["consts"], blur=BC, ndl=NL)
    app.mMainPassCB, app.mSsaoCB = PassConstants(), SsaoConstants()
    C.memmove(C.addressof(app.mMainPassCB), open(d + "/pass_cb_point.bin", "rb").read(), C.sizeof(app.mMainPassCB))
    C.memmove(C.addressof(app.mSsaoCB), open(d + "/ssao_cb_point.bin", "rb").read(), C.sizeof(app.mSsaoCB))
    app.pcfSearchRadius = built_lib.lib.crychic_pcf_search_radius(SD, 1)
    app.set_point_lights(points)
    app.set_point_shadows(COUNT, dim=DIM, z_near=0.5)
    app.mPointShadowMaps.copy_(torch.from_numpy(cubes.view(np.int32)))
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(out, app.mBackBuffer.cpu().numpy())
    app.set_point_shadows(0)
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(out0, app.mBackBuffer.cpu().numpy())
    assert not np.array_equal(out, out0)
    ctx.close()

    sh = np.fromfile(d + "/scene_point.bin", dtype=np.uint8).reshape(H, W, 4).astype(np.int32)
    un = np.fromfile(d + "/scene_point_none.bin", dtype=np.uint8).reshape(H, W, 4).astype(np.int32)
    faces = np.fromfile(d + "/scene_pointmap0.bin", dtype=np.uint32)
    assert (faces < 0xFFFFFF).mean() > 0.2                                  # the light sees the boxes and the grid
    assert (sh <= un).all() and (sh < un).any()
