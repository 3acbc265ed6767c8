"""The chain of passes behind the lighting pass through the C++ veneer (tests/cpp/post_chain_driver.cpp):

    lighting -> fog (in place) -> temporal anti-aliasing -> depth of field -> motion blur -> bloom -> anti-aliasing.

For each switch subset the driver draws -- none, each alone, every pair of buffered stages (so every stage behind every possible
nearest stage in front of it), all five, each with and without the fog -- and both of its frames, every set stage's buffer equals
that pass's checker over the buffer of the nearest set stage in front of it (the back buffer if there is none), Present wrote the last
set stage's buffer, and with all switches off again the frame is the first plain one."""
import numpy as np
import pytest

import bloom_lib
import dof_lib
import motion_blur_lib as mbl
import post_aa_lib as aa
import taa_lib as ta
from test_cpp_veneer import build_driver, run_driver

FOG, TAA, DOF, MB, BLOOM, AA = 1, 2, 4, 8, 16, 32      # the driver's mask bits, in the chain's order
STAGES = ((TAA, "taa"), (DOF, "dof"), (MB, "mb"), (BLOOM, "bloom"), (AA, "aa"))
MASKS = [m for m in range(64) if bin(m & ~FOG).count("1") <= 2 or m | FOG == 63]


def test_the_masks_cover_every_stage_behind_every_source():
    pairs = set()
    for m in MASKS:
        front = "back"
        for bit, name in STAGES:
            if m & bit:
                pairs.add((front, name, bool(m & FOG)))
                front = name
    names = ["back"] + [name for _, name in STAGES]
    want = {(names[i], names[j], fog) for i in range(6) for j in range(i + 1, 6) for fog in (False, True)}
    assert len(want) == 30 and pairs == want
    assert {0, 63} <= set(MASKS) and all(1 << k in MASKS for k in range(6))


def test_post_chain_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("post_chain_driver"))


@pytest.mark.gpu
def test_veneer_post_chain(built_lib, tmp_path):
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, _ = run_driver("post_chain_driver", tmp_path, W, H, SD, CD, BC, NL, "post chain driver ok %dx%d, %d subsets" % (W, H, len(MASKS)))

    def frame(name, m, k):
        return np.fromfile("%s/%s_%d_%d.bin" % (d, name, m, k), np.uint8).reshape(H, W, 4)

    def apply(name, m, k, src):
        """The checker's frame of stage `name` of mask m's frame k over `src`."""
        depth = np.fromfile("%s/depth_%d_%d.bin" % (d, m, k), np.uint32).reshape(H, W)
        cb = np.fromfile("%s/cb_%d_%d.bin" % (d, m, k), np.uint8).tobytes()
        ivp = np.frombuffer(cb, np.float32)[80:96]              # PassConstants::InvViewProj
        mats = np.fromfile("%s/mats_%d_%d.bin" % (d, m, k), np.float32).reshape(4, 16)
        if name == "taa":
            hist = np.fromfile("%s/hist_%d_%d.bin" % (d, m, k), np.uint16).reshape(H, W, 4)
            if k == 0:                                          # a reset frame, and no previous camera
                assert np.array_equal(mats[1], mats[0]) and np.array_equal(hist, src.astype(np.uint16) * 256), (m, k)
                return src
            assert not np.array_equal(mats[1], mats[0]), "the camera strafes before the second frame"
            before = np.fromfile("%s/hist_%d_%d.bin" % (d, m, k - 1), np.uint16).reshape(H, W, 4)
            out, want_hist, _ = ta.checker(ta.Case("chain", ivp, mats[0], mats[1], depth, src, before))
            assert np.array_equal(hist, want_hist), (m, k)
            return out
        if name == "dof":
            return dof_lib.checker(dof_lib.Frame.from_pass_cb(cb, depth), src)[0]
        if name == "mb":
            assert np.array_equal(mats[3], mats[2]) == (k == 0), "no previous camera on the first frame, a strafe before the second"
            case = mbl.Case("chain", ivp, mats[2], mats[3], depth, src)
            return mbl.checker_gather(case, mbl.checker_velocity(case)[0])
        if name == "bloom":
            return bloom_lib.checker(src, bloom_lib.SCENE_PARAMS)[0]
        return aa.checker(src)[0]

    changed = set()
    for m in MASKS:
        for k in range(2):
            back = frame("back", m, k)
            assert np.array_equal(back, frame("back", m & (FOG | TAA), k)), "the back buffer depends on the fog and the jitter alone"
            if m & FOG:
                assert not np.array_equal(back, frame("back", m & TAA, k)), "the fog left the frame alone"
            src = back
            for bit, name in STAGES:
                if m & bit:
                    got = frame(name, m, k)
                    assert np.array_equal(got, apply(name, m, k, src)), "mask %d, frame %d: %s did not read the stage in front of it" % (m, k, name)
                    if not np.array_equal(got, src):
                        changed.add(name)
                    src = got
            ppm = np.fromfile("%s/present_%d_%d.ppm" % (d, m, k), np.uint8)
            assert np.array_equal(ppm[-W * H * 3:].reshape(H, W, 3), src[..., :3]), "mask %d, frame %d: Present did not write the last stage" % (m, k)
    assert changed == {name for _, name in STAGES}, "a stage that never changes its input cannot be seen to be routed: %s" % sorted(changed)
    assert np.array_equal(np.fromfile(d + "/plain_again.bin", np.uint8).reshape(H, W, 4), frame("back", 0, 0))
