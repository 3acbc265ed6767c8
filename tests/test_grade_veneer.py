"""CRYCHIC::SetColourGrade, SetColourGradeLut and LoadColourGradeLut through the C++ veneer (tests/cpp/grade_driver.cpp): with the stage
on, its buffer equals the checker (tests/grade_ref) over the plain frame the application rendered, through the table each setter was
given, and the back buffer stays the plain frame; behind the bloom it is the checker over that pass's buffer, and the anti-aliased
buffer is the anti-aliasing checker's frame over it; with it off the frame is the plain one again; bad tables are refused and a strip
with it on throws."""
import ctypes as C
import os

import numpy as np
import pytest

import grade_lib as gl
import post_aa_lib as aa
from test_cpp_veneer import build_driver, run_driver

WARM = dict(slope=(1.2, 1.0, 0.8), offset=(0.03, 0.0, -0.02), power=(0.9, 1.0, 1.2), saturation=1.3)       # the look the driver sets


def test_grade_driver_compiles(built_lib):
    assert os.path.exists(build_driver("grade_driver"))


@pytest.mark.gpu
def test_veneer_colour_grade(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    lut5, lut17 = gl.corpus_lut(5), gl.corpus_lut(17).copy()
    lut17[..., 3] = 255
    lut5.tofile(str(tmp_path / "lut5.bin"))
    gl.write_cube(tmp_path / "look.cube", lut17, "\r\n")
    (tmp_path / "one_d.cube").write_text("LUT_1D_SIZE 4\n0 0 0\n")
    d, frame = run_driver("grade_driver", tmp_path, W, H, SD, CD, BC, NL, "grade driver ok")
    plain = frame("plain.bin")
    warm = np.zeros((33, 33, 33, 4), np.uint8)
    q = built_lib.GradeParams.default(**WARM)
    built_lib.check(built_lib.lib.crychic_grade_build_lut(C.byref(q), 33, warm.ctypes.data, warm.nbytes))
    want = gl.checker(plain, warm)
    assert not np.array_equal(want, plain), "the look changes nothing on this scene"
    assert np.array_equal(frame("grade_cdl.bin"), want)
    assert np.array_equal(frame("grade_cdl_again.bin"), want), "a refused table changed the stage"
    assert np.array_equal(frame("grade_frame.bin"), plain), "the back buffer is the plain frame"
    assert np.array_equal(frame("grade_lut5.bin"), gl.checker(plain, lut5))
    assert np.array_equal(frame("grade_cube.bin"), gl.checker(plain, lut17))
    bloomed = frame("grade_bloom_in.bin")
    behind = gl.checker(bloomed, lut17)
    assert np.array_equal(frame("grade_bloom.bin"), behind)
    assert np.array_equal(frame("grade_bloom_aa.bin"), aa.checker(behind)[0])
    assert np.array_equal(frame("plain_again.bin"), plain)
