"""CRYCHIC::SetTemporalAA through the C++ veneer (tests/cpp/taa_driver.cpp): the first frame with the switch on, and the first after a
resize, is a reset frame; every later frame's buffer and history equal the checker (tests/taa_ref) and the library called from Python
over what the application rendered and the matrices it kept; the jitter follows crychic_taa_jitter and moves the frame; the depth of
field and the anti-aliasing read the pass's buffer; with it off the frame is the plain one again; bad parameters are refused and a
strip with it on throws."""
import numpy as np
import pytest

import taa_lib as ta
from test_cpp_veneer import build_driver, run_driver

BLEND = 64          # the caller's blend the driver sets for its five frames


def test_taa_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("taa_driver"))


@pytest.mark.gpu
def test_veneer_taa(built_lib, tmp_path):
    import torch
    import post_aa_lib as aa
    from crychic_renderer_amd import Context
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    d, frame = run_driver("taa_driver", tmp_path, W, H, SD, CD, BC, NL, "taa driver ok")

    def record(tag):
        m = np.fromfile(d + "/mats_%s.bin" % tag, np.float32)
        return dict(img=frame("in_%s.bin" % tag), depth=np.fromfile(d + "/depth_%s.bin" % tag, np.uint32).reshape(H, W), taa=frame("taa_%s.bin" % tag),
                    hist=np.fromfile(d + "/hist_%s.bin" % tag, np.uint16).reshape(H, W, 4), ivp=m[:16], cur=m[16:32], prev=m[32:48], jitter=tuple(m[48:50]))
    plain = frame("plain.bin")
    rec = [record(str(k)) for k in range(5)]
    # frame 0 is a reset frame: the jittered frame itself
    assert np.array_equal(rec[0]["taa"], rec[0]["img"]) and np.array_equal(rec[0]["hist"], rec[0]["img"].astype(np.uint16) * 256)
    assert np.array_equal(rec[0]["prev"], rec[0]["cur"])
    ctx = Context(0)
    try:
        for k in range(5):
            assert rec[k]["jitter"] == tuple(np.float32(v) for v in ta.jitter(k)), k
            assert not np.array_equal(rec[k]["img"], plain), "the jitter does not move the frame"
            if k == 0:
                continue
            assert np.array_equal(rec[k]["prev"], rec[k - 1]["cur"])
            assert np.array_equal(rec[k]["cur"], rec[k - 1]["cur"]) == (k < 2), "the camera strafes from frame 2 on"
            case = ta.Case("veneer%d" % k, rec[k]["ivp"], rec[k]["cur"], rec[k]["prev"], rec[k]["depth"], rec[k]["img"], rec[k - 1]["hist"], blend=BLEND)
            out, hist, branch = ta.checker(case)
            assert (branch & ta.B_HISTORY).any() and np.array_equal(rec[k]["taa"], out) and np.array_equal(rec[k]["hist"], hist), k
            dout, dhist = ta.run_device((built_lib, ctx, torch), case)
            assert np.array_equal(dout, out) and np.array_equal(dhist, hist), k
    finally:
        ctx.close()
    # a resize: a reset frame again
    rs = record("resized")
    assert np.array_equal(rs["taa"], rs["img"]) and np.array_equal(rs["hist"], rs["img"].astype(np.uint16) * 256) and np.array_equal(rs["prev"], rs["cur"])
    # the defaults, in front of the depth of field and the anti-aliasing
    ch = record("chain")
    case = ta.Case("chain", ch["ivp"], ch["cur"], ch["prev"], ch["depth"], ch["img"], rs["hist"])
    out, hist, _ = ta.checker(case)
    assert np.array_equal(ch["taa"], out) and np.array_equal(ch["hist"], hist)
    blurred = frame("chain_dof.bin")
    assert not np.array_equal(blurred, out) and not np.array_equal(blurred, ch["img"])
    assert np.array_equal(frame("chain_aa.bin"), aa.checker(blurred)[0])
    assert np.array_equal(frame("plain_again.bin"), plain)
