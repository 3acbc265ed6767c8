"""CRYCHIC::SetDepthOfField through the C++ veneer (tests/cpp/dof_driver.cpp): with the switch on, the pass's buffer equals the checker
(tests/dof_ref) over the plain frame, the depth plane and the pass constants the application rendered, and the back buffer stays the
plain frame; with the anti-aliasing on as well, the anti-aliased buffer is the anti-aliasing checker's frame over the blurred one;
with it off the frame is the plain one again; a bad parameter is refused and a strip with it on throws."""
import numpy as np
import pytest

import dof_lib as dl
import post_aa_lib as aa
from test_cpp_veneer import build_driver, run_driver


def test_dof_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("dof_driver"))


@pytest.mark.gpu
def test_veneer_depth_of_field(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, frame = run_driver("dof_driver", tmp_path, W, H, SD, CD, BC, NL, "dof driver ok")
    plain = frame("plain.bin")
    depth = np.fromfile(d + "/depth.bin", np.uint32).reshape(H, W)
    f = dl.Frame.from_pass_cb(np.fromfile(d + "/pass_cb.bin", np.uint8).tobytes(), depth)
    want, n = dl.checker(f, plain)
    assert n["k_interior"] > 0 and n["behind"] > 0 and not np.array_equal(want, plain), "the scene is all in focus"
    assert np.array_equal(frame("dof.bin"), want)
    assert np.array_equal(frame("dof_frame.bin"), plain), "the back buffer is the previous frame"
    want5, _ = dl.checker(f, plain, dict(focus=30.0, aperture=20.0, radius=5))
    assert not np.array_equal(want5, want) and np.array_equal(frame("dof_params.bin"), want5)
    assert np.array_equal(frame("dof_aa.bin"), aa.checker(want)[0])
    assert np.array_equal(frame("plain_again.bin"), plain)
