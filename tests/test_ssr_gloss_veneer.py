"""CRYCHIC::SetScreenSpaceReflectionGloss through the C++ veneer (tests/cpp/ssr_gloss_driver.cpp): with both switches on, the pass's
buffer equals the checker (tests/ssr_gloss_ref) over the plain frame and the depth plane, G-buffer and pass constants the application
rendered, the pyramid equals the checker's, and the back buffer stays the plain frame; the default parameters are the sharp pass; in
front of the fog the pass's buffer is the fog checker's frame over that; Present writes the pass's buffer; after a resize and back the
frame is the same; with the gloss off the reflections are the sharp ones again and with both off the frame is the plain one; a bad
parameter is refused and the gloss without the reflections throws."""
import numpy as np
import pytest

import fog_lib as fg
import ssr_gloss_lib as gl
import ssr_lib as sl
from test_cpp_veneer import build_driver, run_driver


def test_ssr_gloss_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("ssr_gloss_driver"))


@pytest.mark.gpu
def test_veneer_ssr_gloss(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, frame = run_driver("ssr_gloss_driver", tmp_path, W, H, SD, CD, BC, NL, "ssr gloss driver ok")
    plain = frame("plain.bin")
    depth = np.fromfile(d + "/depth.bin", np.uint32).reshape(H, W)
    g = [np.fromfile(d + "/g%d.bin" % k, np.float32).reshape(H, W, 4) for k in range(3)]
    pcb = np.fromfile(d + "/pass_cb.bin", np.uint8).tobytes()
    f = sl.Frame.from_pass_cb(pcb, g[0], g[1], g[2], depth)
    sharp, n, _ = sl.checker(f, plain)
    assert n["hit_first"] + n["hit_later"] > 0 and not np.array_equal(sharp, plain), "the scene reflects nothing"
    assert np.array_equal(frame("ssr.bin"), sharp)
    assert np.array_equal(frame("gloss_default.bin"), gl.checker(f, plain)[0]) and gl.GLOSS_DEFAULTS["coneScale"] == 0
    mine = dict(coneScale=1.0, levels=5)
    want, n, _ = gl.checker(f, plain, None, mine)
    assert n["lq_positive"] > 0 and n["f_positive"] > 0 and not np.array_equal(want, sharp), "the cone changes nothing"
    assert np.array_equal(frame("gloss.bin"), want)
    assert np.array_equal(frame("gloss_back.bin"), plain)
    pyr = np.fromfile(d + "/pyramid.bin", np.uint8)
    ref = gl.pyramid(plain, 5)
    views, ref_views = gl.level_views(pyr, W, H, 5), gl.level_views(ref, W, H, 5)
    assert len(views) == 5 and all(np.array_equal(a, b) for a, b in zip(views[1:], ref_views[1:]))
    assert np.array_equal(np.fromfile(d + "/present_gloss.ppm", np.uint8)[-W * H * 3:].reshape(H, W, 3), want[..., :3])
    maps = np.stack([np.fromfile(d + "/shadow%d.bin" % j, np.uint32).reshape(SD, SD) for j in range(4)])
    fogged, _ = fg.checker(fg.Frame.from_pass_cb(pcb, depth, maps), want)
    assert not np.array_equal(fogged, want) and np.array_equal(frame("gloss_fog.bin"), fogged)
    assert np.array_equal(frame("gloss_resized.bin"), want)
    assert np.array_equal(frame("ssr_again.bin"), sharp)
    assert np.array_equal(frame("plain_again.bin"), plain)
