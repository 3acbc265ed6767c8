"""The four depth-reading post passes on the device against the float64 / int64 restatements of tests/post_restate.py, directly: the
assertions of tests/test_post_restate_host.py applied to the device's own outputs over the cached corpus cases of at most 70 x 38
pixels and the scene frames of the physical anchor; and the long and thin frames, device against C checker byte for byte behind the
guard bytes.  The caps on the undecided, marginal and inexact shares depend on the cases and the restatement alone: the CPU tier holds
them over the whole corpus, and they are not asserted again on this subset of it."""
import numpy as np
import pytest

import dof_lib as dl
import fog_lib as fg
import motion_blur_lib as mbl
import taa_lib as tl
import test_dof_gpu
import test_fog_gpu
import test_post_restate_host as host
from post_pass_lib import dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu

TINY = 70 * 38
ANCHOR_CAMERA = "mix"


def tiny(cases, pixels):
    return [c for c in cases if pixels(c) <= TINY]


def mb_anchors():
    return [host.anchor_motion_blur_case(W, H, ANCHOR_CAMERA) for W, H in host.ANCHOR_SIZES]


def taa_anchors():
    return [host.anchor_taa_case(W, H, ANCHOR_CAMERA) for W, H in host.ANCHOR_SIZES]


def dof_anchors():
    """The scene frames' depth planes and projection under the default parameters."""
    anchors = []
    for W, H in host.ANCHOR_SIZES:
        s = host.anchor_scene(W, H)
        img = np.random.default_rng(26).integers(0, 256, (H, W, 4), dtype=np.uint8)
        anchors.append(("anchor_%dx%d" % (W, H), dl.Frame((s["A"], s["B"]), s["depth"]), img, "default", "rendered"))
    return anchors


def fog_anchors():
    """The 128 x 96 scene frame with its rendered cascades is the corpus's own scene128_default; the 70 x 38 one is rendered here."""
    from crychic_renderer_amd import scene
    planes = scene.make_scene(70, 38, shadow_dim=64, cube_dim=8, device="cpu")
    frame = fg.Frame.from_pass_cb(planes["consts"].pass_cb, planes["depth"].numpy().view(np.uint32), planes["shadow"].numpy().view(np.uint32))
    img = np.random.default_rng(26).integers(0, 256, (38, 70, 4), dtype=np.uint8)
    return [c for c in host.fog_cases() if c[0] == "scene128_default"] + [("anchor_70x38", frame, img, "default", ("rendered", "rendered"))]


def mb_gpu_cases():
    return tiny(host.mb_cases(), lambda c: c.W * c.H) + mb_anchors()


def taa_gpu_cases():
    return tiny(host.taa_cases(), lambda c: c.W * c.H) + taa_anchors()


def dof_gpu_cases():
    return tiny(host.dof_cases(), lambda c: c[2].shape[0] * c[2].shape[1]) + dof_anchors()


def fog_gpu_cases():
    return tiny(host.fog_cases(), lambda c: c[2].shape[0] * c[2].shape[1]) + fog_anchors()


def test_motion_blur_device_meets_the_restatement(dev):
    """The device's workspace and frame: step A within 1 of the float64 value under the share cap, steps A' and B from the device's
    own velocity plane in exact integers; and on the scene frames the device's words against the velocity of the true points."""
    anchors = mb_anchors()
    got = {}

    def device(case):
        if case.name not in got:
            got[case.name] = mbl.run_device(dev, case)
        return got[case.name]

    fails, shares = host.judge_motion_blur(device, mb_gpu_cases())
    host.report("motion blur, device", shares)
    assert not fails, fails
    for (W, H), case in zip(host.ANCHOR_SIZES, anchors):
        words = mbl.velocity_words(device(case)[0], W, H)[0]
        assert host.anchor_velocity_excess(host.anchor_scene(W, H), case, words) <= 0.5 + host.ANCHOR_SLACK


def test_taa_device_meets_the_restatement(dev):
    """The device's out and history_out, whole frames and the row range [2, H - 2); and on the scene frames the device's history
    position against where the true point was."""
    anchors = taa_anchors()
    fails, shares = host.judge_taa(lambda case, row0, rows: tl.run_device(dev, case, row0, rows), taa_gpu_cases(), input_caps=False)
    host.report("temporal anti-aliasing, device", shares)
    assert not fails, fails
    for (W, H), case in zip(host.ANCHOR_SIZES, anchors):
        n, worst = host.anchor_history_excess(host.anchor_scene(W, H, (0.25, -0.375)), case, tl.run_device(dev, case)[1])
        assert n > W * H // 4 and worst <= host.ANCHOR_SLACK


def test_dof_device_meets_the_restatement(dev):
    """The device's frame against the back end on the checker's c plane (every pixel) and against the whole restatement (every pixel
    whose disc holds no marginal texel); the scene frames under the default parameters."""
    def device(case, row0, rows):
        name, frame, img, pname, _ = case
        out = test_dof_gpu.run_device(dev, frame, img, dl.PARAM_SETS[pname], row0, rows)
        coc = None
        if rows is None:
            coc = host.cached(("dof_coc", name), lambda: dl.checker(frame, img, dl.PARAM_SETS[pname], coc=True)[2])
        return out, coc

    fails, shares = host.judge_dof(device, dof_gpu_cases(), input_caps=False)
    host.report("depth of field, device", shares)
    assert not fails, fails


def test_fog_device_lies_in_the_restatements_interval(dev):
    """Every R, G, B byte of the device's frame in [lo, hi], the two scene frames with their rendered cascades included."""
    fails, shares = host.judge_fog(lambda case: test_fog_gpu.run_device(dev, case[1], case[2], fg.PARAM_SETS[case[3]]), fog_gpu_cases(), input_caps=False)
    host.report("fog, device", shares)
    assert not fails, fails


@pytest.mark.parametrize("W,H", host.THIN_SIZES)
def test_long_thin_frames_equal_the_checkers(dev, W, H):
    """4100 and 65600 columns or rows, about 131 000 pixels each: no entry refuses them (the header's limits are 2^28 pixels and, for
    the two reprojecting passes, 2^22 columns or rows), and the device equals the checker in every byte; run_device checks the guard
    bytes and the inputs."""
    case, want = host.thin_case("motion_blur", W, H)
    ws, out = mbl.run_device(dev, case)
    assert np.array_equal(ws, want[0]), "motion blur: the workspace"
    assert np.array_equal(out, want[1]), "motion blur: the frame"
    case, want = host.thin_case("taa", W, H)
    out, hout = tl.run_device(dev, case)
    assert np.array_equal(out, want[0]) and np.array_equal(hout, want[1]), "temporal anti-aliasing"
    (frame, img, params), want = host.thin_case("dof", W, H)
    assert np.array_equal(test_dof_gpu.run_device(dev, frame, img, params), want), "depth of field"
    (frame, img, params), want = host.thin_case("fog", W, H)
    assert np.array_equal(test_fog_gpu.run_device(dev, frame, img, params), want), "fog"
