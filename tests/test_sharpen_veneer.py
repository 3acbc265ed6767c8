"""CRYCHIC::SetSharpening through the C++ veneer (tests/cpp/sharpen_driver.cpp): with the stage on, its buffer equals the checker
(tests/sharpen_ref) over the plain frame the application rendered, and the back buffer stays the plain frame; behind the temporal
anti-aliasing it is the checker over that pass's resolved frame; behind the temporal upsampling it runs at the display size and the
anti-aliased buffer is the anti-aliasing checker's frame over it; with it off the frame is the plain one again; bad parameters are
refused and a strip with it on throws, naming the stage."""
import os

import numpy as np
import pytest

import post_aa_lib as aa
import sharpen_lib as sl
from test_cpp_veneer import build_driver, run_driver


def test_sharpen_driver_compiles(built_lib):
    assert os.path.exists(build_driver("sharpen_driver"))


@pytest.mark.gpu
def test_veneer_sharpening(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    WO, HO = 192, 144
    d, frame = run_driver("sharpen_driver", tmp_path, W, H, SD, CD, BC, NL, "sharpen driver ok", extra=(WO, HO))
    plain = frame("plain.bin")
    default = built_lib.SharpenParams.default()
    want = sl.checker(plain, default.strength, default.limit)
    strong = sl.checker(plain, sl.MAX_STRENGTH, sl.MAX_LIMIT)
    assert not np.array_equal(strong, plain), "the pass changes nothing on this scene"
    assert np.array_equal(frame("sharp.bin"), want)
    assert np.array_equal(frame("sharp_again.bin"), want), "refused parameters changed the stage"
    assert np.array_equal(frame("sharp_frame.bin"), plain), "the back buffer is the plain frame"
    resolved = frame("sharp_taa_in.bin")
    assert np.array_equal(frame("sharp_taa.bin"), sl.checker(resolved, sl.MAX_STRENGTH, sl.MAX_LIMIT))
    up = np.fromfile(d + "/sharp_up_in.bin", np.uint8).reshape(HO, WO, 4)
    behind = sl.checker(up, sl.MAX_STRENGTH, sl.MAX_LIMIT)
    assert not np.array_equal(behind, up)
    assert np.array_equal(np.fromfile(d + "/sharp_up.bin", np.uint8).reshape(HO, WO, 4), behind)
    assert np.array_equal(np.fromfile(d + "/sharp_up_aa.bin", np.uint8).reshape(HO, WO, 4), aa.checker(behind)[0])
    assert np.array_equal(frame("plain_again.bin"), plain)
