"""CRYCHIC::SetScreenSpaceReflections through the C++ veneer (tests/cpp/ssr_driver.cpp): with the switch on, the pass's buffer equals
the checker (tests/ssr_ref) over the plain frame and the depth plane, G-buffer and pass constants the application rendered, and the
back buffer stays the plain frame; in front of the fog the pass's buffer is the fog checker's frame over that, in front of the depth
of field the second buffer is the depth-of-field checker's; Present writes the last stage's buffer; with the switch off the frame is
the plain one again; a bad parameter is refused and a strip with it on throws."""
import numpy as np
import pytest

import dof_lib as df
import fog_lib as fg
import ssr_lib as sl
from test_cpp_veneer import build_driver, run_driver


def test_ssr_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("ssr_driver"))


@pytest.mark.gpu
def test_veneer_ssr(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, frame = run_driver("ssr_driver", tmp_path, W, H, SD, CD, BC, NL, "ssr driver ok")
    plain = frame("plain.bin")
    depth = np.fromfile(d + "/depth.bin", np.uint32).reshape(H, W)
    g = [np.fromfile(d + "/g%d.bin" % k, np.float32).reshape(H, W, 4) for k in range(3)]
    pcb = np.fromfile(d + "/pass_cb.bin", np.uint8).tobytes()
    f = sl.Frame.from_pass_cb(pcb, g[0], g[1], g[2], depth)
    want, n, _ = sl.checker(f, plain)
    assert n["hit_first"] + n["hit_later"] > 0 and not np.array_equal(want, plain), "the scene reflects nothing"
    assert np.array_equal(frame("ssr.bin"), want)
    assert np.array_equal(frame("ssr_back.bin"), plain)

    def present(name):
        return np.fromfile(d + "/" + name, np.uint8)[-W * H * 3:].reshape(H, W, 3)
    assert np.array_equal(present("present_ssr.ppm"), want[..., :3])
    mine = dict(sl.DEFAULTS, maxDistance=12.0, thickness=1.5, maxRoughness=1.0, steps=48, edgeFade=8, intensity=200)
    want_mine, _, _ = sl.checker(f, plain, mine)
    assert not np.array_equal(want_mine, want) and np.array_equal(frame("ssr_params.bin"), want_mine)
    # in front of the fog
    maps = np.stack([np.fromfile(d + "/shadow%d.bin" % j, np.uint32).reshape(SD, SD) for j in range(4)])
    fogged, _ = fg.checker(fg.Frame.from_pass_cb(pcb, depth, maps), want)
    assert not np.array_equal(fogged, want) and np.array_equal(frame("ssr_fog.bin"), fogged)
    assert np.array_equal(frame("ssr_fog_back.bin"), plain)
    # in front of the depth of field
    assert np.array_equal(frame("ssr_dof_front.bin"), want)
    blurred, _ = df.checker(df.Frame.from_pass_cb(pcb, depth), want)
    assert not np.array_equal(blurred, want) and np.array_equal(frame("ssr_dof.bin"), blurred)
    assert np.array_equal(present("present_dof.ppm"), blurred[..., :3])
    assert np.array_equal(frame("plain_again.bin"), plain)
