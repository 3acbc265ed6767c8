"""CRYCHIC::SetAntiAliasing through the C++ veneer (tests/cpp/post_aa_driver.cpp): with the switch on, Present writes the anti-aliased
frame, which equals the checker (tests/post_aa_ref) on the plain frame; with it off the frame is the oracle's, as before; a strip with
it on throws."""
import ctypes as C

import numpy as np
import pytest

import post_aa_lib as aa
from test_cpp_veneer import build_driver, run_driver


def test_post_aa_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("post_aa_driver"))


def read_ppm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P6"
        w, h = (int(v) for v in f.readline().split())
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(), np.uint8).reshape(h, w, 3)


@pytest.mark.gpu
def test_veneer_anti_aliasing(built_lib, oracle, tmp_path):
    import raster_util
    import torch
    from crychic_renderer_amd import geometry as g, scene
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, frame = run_driver("post_aa_driver", tmp_path, W, H, SD, CD, BC, NL, "post aa driver ok")
    cube = scene.make_cubemap(CD, torch.device("cpu")).numpy()
    plain = frame("plain.bin")
    # with the switch off the frame is today's: the all-CPU oracle frame of the built-in scene
    consts = raster_util.frame_constants(W, H, SD)
    cam = scene.default_camera(W, H)
    items, shadow_items = g.cascade_scene_items(cull_camera=cam), g.cascade_scene_items(shadow_layer=True, cull_camera=cam)
    ref = raster_util.oracle_frame(oracle, consts, items, shadow_items, g.reference_materials(), None, W, H, SD, cube, BC, NL,
                                   built_lib.lib.crychic_pcf_search_radius(SD, 1))
    assert np.array_equal(plain, ref["rgba8"])
    assert np.array_equal(read_ppm(d + "/plain.ppm"), plain[..., :3])
    # with it on: the back buffer is untouched, the second buffer is the checker's frame, and Present writes it
    want, n = aa.checker(plain)
    assert n["horizontal"] + n["vertical"] > 0 and not np.array_equal(want, plain), "the scene has no edge to smooth"
    assert np.array_equal(frame("frame.bin"), plain)
    assert np.array_equal(frame("aa.bin"), want)
    assert np.array_equal(read_ppm(d + "/aa.ppm"), want[..., :3])
    assert np.array_equal(frame("resized_aa.bin"), want)
    # and off again
    assert np.array_equal(frame("plain_again.bin"), plain)
    assert np.array_equal(read_ppm(d + "/plain_again.ppm"), plain[..., :3])
