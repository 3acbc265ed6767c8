"""CRYCHIC::SetFog through the C++ veneer (tests/cpp/fog_driver.cpp): with the switch on, the back buffer equals the checker
(tests/fog_ref) over the plain frame and the depth plane, pass constants and cascade maps the application rendered; with the
anti-aliasing on as well, the second back buffer is the anti-aliasing checker's frame over the fogged one; with it off the frame is
the plain one again; a bad parameter is refused and a strip with it on throws."""
import numpy as np
import pytest

import fog_lib as fg
import post_aa_lib as aa
from test_cpp_veneer import build_driver, run_driver


def test_fog_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("fog_driver"))


@pytest.mark.gpu
def test_veneer_fog(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, frame = run_driver("fog_driver", tmp_path, W, H, SD, CD, BC, NL, "fog driver ok")
    plain = frame("plain.bin")
    depth = np.fromfile(d + "/depth.bin", np.uint32).reshape(H, W)
    maps = np.stack([np.fromfile(d + "/shadow%d.bin" % j, np.uint32).reshape(SD, SD) for j in range(4)])
    f = fg.Frame.from_pass_cb(np.fromfile(d + "/pass_cb.bin", np.uint8).tobytes(), depth, maps)
    want, n = fg.checker(f, plain)
    assert n["lit"] > 0 and n["shadowed"] > 0 and not np.array_equal(want, plain), "the scene has no shaft"
    assert np.array_equal(frame("fog.bin"), want)
    want7, _ = fg.checker(f, plain, dict(fg.DEFAULTS, density=float(np.float32(0.08)), steps=7, sun=(250, 200, 90)))
    assert not np.array_equal(want7, want) and np.array_equal(frame("fog_params.bin"), want7)
    assert np.array_equal(frame("fog_frame.bin"), want)
    assert np.array_equal(frame("fog_aa.bin"), aa.checker(want)[0])
    assert np.array_equal(frame("plain_again.bin"), plain)
