"""The C++ veneer's shadowed spot lights (include/crychic/CRYCHIC.h SetSpotShadows): tests/cpp/local_lights_driver.cpp renders
through CRYCHIC::Draw and its frames are compared with the Python path's (the C entries) bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from local_lights_util import DRIVER_FRAME, _app, _device_scene, run_local_lights_driver


def test_spot_shadow_driver_compiles(built_lib):
    """CPU tier: the veneer with SetLocalLights and SetSpotShadows compiles and links against libcrychic_hip.so."""
    import test_cpp_veneer
    assert os.path.exists(test_cpp_veneer.build_driver("local_lights_driver"))


@pytest.mark.gpu
def test_veneer_set_spot_shadows(built_lib, tmp_path):
    """SetLocalLights + SetSpotShadows(3, 128), then Draw: the frame equals the Python path's (Crychic.set_spot_shadows with the
    same maps) bit for bit; SetSpotShadows(0) gives back the unshadowed frame; the argument errors throw (checked in the driver).
    The built-in scene with its producer passes: the spot map is rendered after the cascades and the shadowed frame is nowhere
    brighter than the unshadowed one, and darker somewhere."""
    import torch
    from crychic_renderer_amd import Context
    from crychic_renderer_amd._lib import PassConstants, SsaoConstants
    F = DRIVER_FRAME
    W, H, SD, BC, NL, COUNT, DIM = F["W"], F["H"], F["SD"], F["BC"], F["NL"], F["COUNT"], F["DIM"]
    d = str(tmp_path)
    pl, _, _, spots, maps = run_local_lights_driver(d)
    out = np.fromfile(d + "/out_shadowed.bin", dtype=np.uint8).reshape(H, W, 4)
    out0 = np.fromfile(d + "/out_noshadow.bin", dtype=np.uint8).reshape(H, W, 4)

    ctx = Context(0)
    _, _, dev = _device_scene(ctx, W, H, SD, F["CD"])
    app = _app(ctx, W, H, dev, pl["consts"], blur=BC, ndl=NL)
    app.mMainPassCB, app.mSsaoCB = PassConstants(), SsaoConstants()
    C.memmove(C.addressof(app.mMainPassCB), open(d + "/pass_cb_shadowed.bin", "rb").read(), C.sizeof(app.mMainPassCB))
    C.memmove(C.addressof(app.mSsaoCB), open(d + "/ssao_cb_shadowed.bin", "rb").read(), C.sizeof(app.mSsaoCB))
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
