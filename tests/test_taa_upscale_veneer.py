"""CRYCHIC::SetTemporalUpscale through the C++ veneer (tests/cpp/taa_upscale_driver.cpp): the first frame with the switch on, and the
first after a resize, is a reset frame; every frame's buffer and history equal the checker (tests/taa_upscale_ref) over what the
application rendered, the matrices and the jitter it kept; the bloom and the anti-aliasing behind it run at the display size, which is
what Present writes; with it off the frame is the plain one again; bad parameters are refused and the four refusals of Draw throw."""
import numpy as np
import pytest

import taa_lib as ta
import taa_upscale_lib as tu
from test_cpp_veneer import build_driver, run_driver

BLEND = 200         # the caller's blend the driver sets for its four frames


def test_taa_upscale_driver_compiles(built_lib):
    import os
    assert os.path.exists(build_driver("taa_upscale_driver"))


@pytest.mark.gpu
def test_veneer_taa_upscale(built_lib, tmp_path):
    import bloom_lib
    import post_aa_lib as aa
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 2, 1
    WO, HO = 192, 144
    d, frame = run_driver("taa_upscale_driver", tmp_path, W, H, SD, CD, BC, NL, "taa upscale driver ok")

    def big(name):
        return np.fromfile(d + "/" + name, np.uint8).reshape(HO, WO, 4)

    def record(tag):
        m = np.fromfile(d + "/mats_%s.bin" % tag, np.float32)
        return dict(img=frame("in_%s.bin" % tag), depth=np.fromfile(d + "/depth_%s.bin" % tag, np.uint32).reshape(H, W), up=big("up_%s.bin" % tag),
                    hist=np.fromfile(d + "/hist_%s.bin" % tag, np.uint16).reshape(HO, WO, 4), ivp=m[:16], cur=m[16:32], prev=m[32:48],
                    jitter=(float(m[48]), float(m[49])))

    def case(r, hist, blend, reset=False):
        return tu.Case("veneer", r["ivp"], r["cur"], r["prev"], r["jitter"], r["depth"], r["img"], (WO, HO), hist, blend, tu.RESET if reset else 0)
    plain = frame("plain.bin")
    rec = [record(str(k)) for k in range(4)]
    assert np.array_equal(rec[0]["prev"], rec[0]["cur"])
    hist = None
    for k in range(4):
        assert rec[k]["jitter"] == tuple(float(np.float32(v)) for v in ta.jitter(k)), k
        assert not np.array_equal(rec[k]["img"], plain), "the jitter does not move the frame"
        if k:
            assert np.array_equal(rec[k]["prev"], rec[k - 1]["cur"])
            assert np.array_equal(rec[k]["cur"], rec[k - 1]["cur"]) == (k < 2), "the camera strafes from frame 2 on"
        out, hist, branch = tu.checker(case(rec[k], hist, BLEND, reset=k == 0))
        assert bool((branch & tu.B_HISTORY).any()) == (k > 0)
        assert np.array_equal(rec[k]["up"], out) and np.array_equal(rec[k]["hist"], hist), k
    # a resize: a reset frame again
    rs = record("resized")
    out, hist, _ = tu.checker(case(rs, None, BLEND, reset=True))
    assert np.array_equal(rs["up"], out) and np.array_equal(rs["hist"], hist) and np.array_equal(rs["prev"], rs["cur"])
    # the defaults, the bloom and the anti-aliasing behind the pass at the display size
    ch = record("chain")
    out, hist, _ = tu.checker(case(ch, rs["hist"], tu.DEFAULT_BLEND))
    assert np.array_equal(ch["up"], out) and np.array_equal(ch["hist"], hist)
    bloomed = bloom_lib.checker(out)[0]
    assert np.array_equal(big("chain_bloom.bin"), bloomed)
    final = aa.checker(bloomed)[0]
    assert np.array_equal(big("chain_aa.bin"), final)
    with open(d + "/final.ppm", "rb") as f:
        ppm = f.read()
    assert ppm.startswith(b"P6\n%d %d\n255\n" % (WO, HO)) and ppm[-WO * HO * 3:] == final[..., :3].tobytes(), "Present writes the finished frame at the display size"
    assert np.array_equal(frame("plain_again.bin"), plain)
