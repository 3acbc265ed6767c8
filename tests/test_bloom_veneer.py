"""CRYCHIC::SetBloom through the C++ veneer (tests/cpp/bloom_driver.cpp): with the switch on, the pass's buffer equals the checker
(tests/bloom_ref) over the plain frame the application rendered, and the back buffer stays the plain frame; behind the depth of field
it is the checker over that pass's buffer, and the anti-aliased buffer is the anti-aliasing checker's frame over it; with it off the
frame is the plain one again; bad parameters are refused and a strip with it on throws."""
import numpy as np
import pytest

import bloom_lib as bl
import post_aa_lib as aa
from test_cpp_veneer import build_driver, run_driver

LOW = dict(threshold=160, intensity=64)         # the caller's parameters the driver sets besides the defaults


def test_bloom_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("bloom_driver"))


@pytest.mark.gpu
def test_veneer_bloom(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, frame = run_driver("bloom_driver", tmp_path, W, H, SD, CD, BC, NL, "bloom driver ok")
    plain = frame("plain.bin")
    want, _, n = bl.checker(plain, LOW)
    assert n["w_interior"] + n["w_full"] > 0 and not np.array_equal(want, plain), "nothing of the scene lies over the threshold"
    assert np.array_equal(frame("bloom.bin"), want)
    assert np.array_equal(frame("bloom_frame.bin"), plain), "the back buffer is the previous frame"
    assert np.array_equal(frame("bloom_default.bin"), bl.checker(plain)[0])
    blurred = frame("bloom_dof_in.bin")
    assert not np.array_equal(blurred, plain)
    behind = bl.checker(blurred, LOW)[0]
    assert np.array_equal(frame("bloom_dof.bin"), behind)
    assert np.array_equal(frame("bloom_dof_aa.bin"), aa.checker(behind)[0])
    assert np.array_equal(frame("plain_again.bin"), plain)
