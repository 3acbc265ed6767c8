"""CRYCHIC::SetMotionBlur through the C++ veneer (tests/cpp/motion_blur_driver.cpp): the first frame with the switch on, and the first
after a resize, has no previous camera and copies the frame; every frame's buffer and workspace equal the checker
(tests/motion_blur_ref) and the library called from Python over what the application rendered and the matrices it kept; the pass reads
the depth of field's buffer and the bloom and the anti-aliasing read the pass's; with it off the frame is the plain one again; bad
parameters are refused and a strip with it on throws."""
import numpy as np
import pytest

import motion_blur_lib as mbl
from test_cpp_veneer import build_driver, run_driver

SHUTTER, SAMPLES, RADIUS = 256, 16, 24          # the caller's parameters the driver sets for its five frames


def test_motion_blur_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("motion_blur_driver"))


@pytest.mark.gpu
def test_veneer_motion_blur(built_lib, tmp_path):
    import torch
    import bloom_lib
    import post_aa_lib as aa
    from crychic_renderer_amd import Context
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, frame = run_driver("motion_blur_driver", tmp_path, W, H, SD, CD, BC, NL, "motion blur driver ok")

    def record(tag):
        m = np.fromfile(d + "/mats_%s.bin" % tag, np.float32)
        return dict(img=frame("in_%s.bin" % tag), depth=np.fromfile(d + "/depth_%s.bin" % tag, np.uint32).reshape(H, W), mb=frame("mb_%s.bin" % tag),
                    ws=np.fromfile(d + "/ws_%s.bin" % tag, np.uint8), ivp=m[:16], cur=m[16:32], prev=m[32:48])
    plain = frame("plain.bin")
    rec = [record(str(k)) for k in range(5)]
    assert np.array_equal(rec[0]["img"], plain), "the pass leaves the back buffer alone and does not jitter"
    ctx = Context(0)
    try:
        for k in range(5):
            assert np.array_equal(rec[k]["prev"], rec[k]["cur"] if k == 0 else rec[k - 1]["cur"]), k
            assert np.array_equal(rec[k]["cur"], rec[k]["prev"]) == (k < 2), "the camera strafes from frame 2 on"
            case = mbl.Case("veneer%d" % k, rec[k]["ivp"], rec[k]["cur"], rec[k]["prev"], rec[k]["depth"], rec[k]["img"], SHUTTER, SAMPLES, RADIUS)
            ws, _ = mbl.checker_velocity(case)
            out = mbl.checker_gather(case, ws)
            assert np.array_equal(out, rec[k]["img"]) == (k < 2), k
            assert np.array_equal(rec[k]["mb"], out) and np.array_equal(rec[k]["ws"], ws), k
            dws, dout = mbl.run_device((built_lib, ctx, torch), case)
            assert np.array_equal(dout, out) and np.array_equal(dws, ws), k
    finally:
        ctx.close()
    # a resize: no previous camera although the camera moved
    rs = record("resized")
    assert np.array_equal(rs["prev"], rs["cur"]) and not np.array_equal(rs["cur"], rec[4]["cur"]) and np.array_equal(rs["mb"], rs["img"])
    # the defaults, behind the depth of field and in front of the bloom and the anti-aliasing
    ch = record("chain")
    assert np.array_equal(ch["prev"], rs["cur"]) and not np.array_equal(ch["cur"], ch["prev"])
    focused = frame("chain_dof.bin")
    assert not np.array_equal(focused, ch["img"])
    case = mbl.Case("chain", ch["ivp"], ch["cur"], ch["prev"], ch["depth"], focused)
    ws, _ = mbl.checker_velocity(case)
    out = mbl.checker_gather(case, ws)
    assert not np.array_equal(out, focused) and np.array_equal(ch["mb"], out) and np.array_equal(ch["ws"], ws)
    bloomed = frame("chain_bloom.bin")
    assert np.array_equal(bloomed, bloom_lib.checker(out)[0])
    assert np.array_equal(frame("chain_aa.bin"), aa.checker(bloomed)[0])
    assert np.array_equal(frame("plain_again.bin"), plain)
