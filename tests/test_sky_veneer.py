"""CRYCHIC::RenderSky and CRYCHIC::SetProceduralSky through the C++ veneer (tests/cpp/sky_driver.cpp): the cube map an explicit
RenderSky binds equals the checker (tests/sky_ref) under the caller's parameters; with SetProceduralSky(true) the bound cube map is the
checker's sky under -Lights[0].Direction of each frame's pass constants, across a turned light; and with neither, the frame is the one
the existing fog driver draws with its switch off."""
import numpy as np
import pytest

import sky_lib as sk
from test_cpp_veneer import build_driver, run_driver


def test_sky_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("sky_driver"))


@pytest.mark.gpu
def test_veneer_sky(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    for sub in ("sky", "fog"):
        (tmp_path / sub).mkdir()
    d, frame = run_driver("sky_driver", tmp_path / "sky", W, H, SD, CD, BC, NL, "sky driver ok")

    def cube(name):
        return np.fromfile(d + "/" + name, np.uint8).reshape(6, CD, CD, 4)
    plain = frame("plain.bin")
    want, _ = sk.checker(CD, dict(sunDir=(0.3, 0.2, -0.8), altitude=1.5, viewSteps=9, sunSteps=5))
    assert np.array_equal(cube("sky_cube.bin"), want), "RenderSky's cube map is not the checker's"
    assert (frame("sky.bin") != plain).any()
    suns = []
    for k in range(2):
        cb = built_lib.PassConstants.from_buffer_copy(np.fromfile(d + "/follow_cb%d.bin" % k, np.uint8).tobytes())
        sun = tuple(float(np.float32(-v)) for v in cb.Lights[0].Direction)
        suns.append(sun)
        want, _ = sk.checker(CD, dict(sunDir=sun))
        assert np.array_equal(cube("follow_cube%d.bin" % k), want), "frame %d: the bound cube map is not the sky under Lights[0]" % k
    assert suns[0] != suns[1] and (cube("follow_cube0.bin") != cube("follow_cube1.bin")).any(), "the light did not turn"
    assert np.array_equal(frame("follow_still.bin"), frame("follow1.bin"))
    assert np.array_equal(cube("off_cube.bin"), cube("follow_cube1.bin")), "turning the switch off re-rendered or unbound the sky"
    # with neither RenderSky nor the switch, the frame is the existing driver's
    d2, frame2 = run_driver("fog_driver", tmp_path / "fog", W, H, SD, CD, BC, NL, "fog driver ok")
    assert np.array_equal(frame2("plain.bin"), plain)
