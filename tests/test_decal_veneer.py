"""CRYCHIC::SetDecals / ClearDecals through the C++ veneer (tests/cpp/decal_driver.cpp): with decals set, the G-buffer planes behind
Draw's producer passes equal the checker (tests/decal_ref) over the planes, the depth plane and the pass constants the application
rendered without them, and the lit frame shows them; cleared, the frame is the plain one again; as a strip, the strip's rows are
decaled and the others are not; too many decals are refused."""
import numpy as np
import pytest

import decal_lib as dl
from test_cpp_veneer import build_driver, run_driver


def test_decal_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("decal_driver"))


@pytest.mark.gpu
def test_veneer_decals(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    R0, RN = 32, 24
    d = str(tmp_path)
    rng = np.random.default_rng(7)
    tex = dl.random_texture(rng, 8, 4, 3)
    tex[0].tofile(d + "/tex.bin")
    # a wide floor decal with every flag and the texture as its own normal map, and a second one over it that changes the albedo alone
    recs = dl.decals_array([
        dl.decal_from_box(dl.floor_world((0.0, 0.0, 0.0), (12.0, 1.0, 12.0)), (8, 4), 0.5, -0.5, texture=0, normalTexture=0, flags=15, roughness=0.2,
                          metalness=0.7, tint=(0.9, 0.4, 0.1)),
        dl.decal_from_box(dl.floor_world((1.0, 0.0, -4.0), (3.0, 1.0, 3.0), yaw=0.4), (8, 4), texture=0, flags=1, opacity=0.5)])
    recs.tofile(d + "/decals.bin")
    d, frame = run_driver("decal_driver", tmp_path, W, H, SD, CD, BC, NL, "decal driver ok", extra=(8, 4, 3, R0, RN))

    def plane(name):
        return np.fromfile(d + "/" + name, np.float32).reshape(H, W, 4)
    f = np.frombuffer(np.fromfile(d + "/pass_cb.bin", np.uint8).tobytes(), np.float32)
    fr = dl.Frame(f[0:16], f[32:48], np.fromfile(d + "/depth.bin", np.uint32).reshape(H, W), plane("g0.bin"), plane("g1.bin"), plane("g2.bin"))
    want, n = dl.checker(fr, "f32", recs, [tex])
    assert n["store_albedo"] > 1000 and n["store_normal"] > 1000 and n["store_metalness"] > 1000, n
    for k in range(3):
        got = np.fromfile(d + "/g%d_decal.bin" % k, np.uint8).reshape(want[k].shape)
        assert np.array_equal(got, want[k]), "G%d differs from the checker in %d bytes" % (k, int((got != want[k]).sum()))
    plain = frame("plain.bin")
    assert int((frame("decal.bin") != plain).any(-1).sum()) > 1000, "the decals do not show in the lit frame"
    assert np.array_equal(frame("plain_again.bin"), plain)
    strip = np.fromfile(d + "/g1_strip.bin", np.uint8).reshape(want[1].shape)
    g1 = fr.planes("f32")[1]
    assert np.array_equal(strip[R0:R0 + RN], want[1][R0:R0 + RN])
    assert np.array_equal(strip[:R0], g1[:R0]) and np.array_equal(strip[R0 + RN:], g1[R0 + RN:])
    assert not np.array_equal(want[1][R0 + RN:], g1[R0 + RN:])          # the rows below the strip would have been decaled too
