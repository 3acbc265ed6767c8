"""The passes behind the lighting pass as Crychic.Draw chains them,

    lighting -> fog (in place) -> temporal anti-aliasing -> depth of field -> motion blur -> bloom -> anti-aliasing,

over all 64 subsets of the six switches: the bytes of every buffer against the same passes issued by hand on a second object, the
library calls by name, the refusal of a strip or a shared draw, and where the finished frame is."""
import numpy as np
import pytest

import bloom_lib
import motion_blur_lib as mbl
from recorder_lib import Recorder

pytestmark = pytest.mark.gpu

SWITCHES = ("fog", "temporalAA", "depthOfField", "motionBlur", "bloom", "antiAliasing")          # in the chain's order
BUFFER = dict(temporalAA="mBackBufferTAA", depthOfField="mBackBufferDoF", motionBlur="mBackBufferMB", bloom="mBackBufferBloom",
              antiAliasing="mBackBufferAA")                                                      # the fog has none: in place on mBackBuffer
SUBSETS = [tuple(s for k, s in enumerate(SWITCHES) if mask >> k & 1) for mask in range(64)]
LIGHTING = ["crychic_draw_hot_path_point_shadows"]
CALLS = dict(fog=["crychic_fog"], temporalAA=["crychic_taa"], depthOfField=["crychic_dof"],      # what each switch alone adds to a Draw()
             motionBlur=["crychic_motion_blur_workspace_bytes", "crychic_motion_blur"], bloom=["crychic_bloom_workspace_bytes", "crychic_bloom"],
             antiAliasing=["crychic_antialias"])
W, H, SD = 128, 96, 256


@pytest.fixture(scope="module")
def chain(built_lib):
    """Two Crychic over the planes of one 128 x 96 synthetic scene -- `app` for Draw(), `hand` whose switches are never set --, the
    frame without a pass, the value of each switch (every stage changes its input on this scene) and the two cameras."""
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, scene
    lib = built_lib
    ctx = Context(0)
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    apps = []
    for _ in range(2):
        a = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
        a.load_scene(planes)
        a.blurCount, a.numDirLights, a.flags = 3, 3, LIGHT_SKY
        apps.append(a)
    app, hand = apps
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.clone()
    values = dict.fromkeys(SWITCHES, True)
    values["bloom"] = lib.BloomParams.default(**bloom_lib.SCENE_PARAMS)
    cur = np.array(app.mMainPassCB.ViewProj[:], np.float32)
    moved = mbl.camera_matrices(W, H, cam=mbl.moved_camera(W, H, dx=-0.3, yaw=0.02))[0]
    for a in apps:                                              # the camera has moved between the two frames
        a.set_frame_view_proj(moved)
        a.set_frame_view_proj(cur)
    yield lib, torch, app, hand, plain, values, cur, moved
    ctx.close()


def set_switches(app, subset, values):
    for s in SWITCHES:
        setattr(app, s, None)
    for s in subset:
        setattr(app, s, values[s])


def issue_by_hand(hand, subset, values, cur, prev, reset):
    """A frame and the stages of `subset` through the public pass methods, each from what the stage in front returned."""
    hand.Draw()
    frame = hand.mBackBuffer
    if "fog" in subset:
        frame = hand.apply_fog(src=frame)
    if "temporalAA" in subset:
        frame = hand.temporal_aa(cur, prev, src=frame, reset=reset)
    if "depthOfField" in subset:
        frame = hand.depth_of_field(src=frame)
    if "motionBlur" in subset:
        frame = hand.motion_blur(cur, prev, src=frame)
    if "bloom" in subset:
        frame = hand.apply_bloom(src=frame, params=values["bloom"])
    if "antiAliasing" in subset:
        frame = hand.antialias(src=frame)
    return frame


def test_every_stage_changes_its_input(chain):
    """The precondition of the tests below: with all six set, every stage's buffer differs from the buffer it read, on both frames --
    but for the temporal pass on its RESET frame, which hands its input on.  A skipped or misrouted stage cannot hide."""
    lib, torch, app, hand, plain, values, cur, moved = chain
    set_switches(app, SWITCHES, values)
    try:
        for frame in range(2):
            app.Draw()
            torch.cuda.synchronize()
            assert not torch.equal(app.mBackBuffer, plain), "fog, frame %d" % frame
            src = app.mBackBuffer
            for s in SWITCHES[1:]:
                out = getattr(app, BUFFER[s])
                assert torch.equal(out, src) == (s == "temporalAA" and frame == 0), "%s, frame %d" % (s, frame)
                src = out
    finally:
        set_switches(app, (), values)


def test_every_subset_leaves_the_bytes_of_the_passes_issued_by_hand(chain):
    lib, torch, app, hand, plain, values, cur, moved = chain
    try:
        for subset in SUBSETS:
            set_switches(app, subset, values)                   # from cleared: the temporal pass's first frame is a RESET frame
            for frame in range(2):
                app.Draw()
                last = issue_by_hand(hand, subset, values, cur, moved, reset=frame == 0)
                torch.cuda.synchronize()
                where = "%s, frame %d" % ("+".join(subset) or "none", frame)
                assert torch.equal(app.mBackBuffer, hand.mBackBuffer), where
                assert torch.equal(app.mBackBuffer, plain) == ("fog" not in subset), where
                stages = [s for s in subset if s != "fog"]
                for s in stages:
                    assert torch.equal(getattr(app, BUFFER[s]), getattr(hand, BUFFER[s])), "%s: %s" % (where, BUFFER[s])
                assert last is (getattr(hand, BUFFER[stages[-1]]) if stages else hand.mBackBuffer), where
                if "temporalAA" in subset:
                    assert torch.equal(app.mTaaHistory[0], hand.mTaaHistory[0]), where
                if "motionBlur" in subset:
                    assert torch.equal(app.mMotionBlurWorkspace, hand.mMotionBlurWorkspace), where
                if "bloom" in subset:
                    assert torch.equal(app.mBloomWorkspace, hand.mBloomWorkspace), where
            assert not hand._post
    finally:
        set_switches(app, (), values)


def test_every_subset_issues_the_calls_of_its_stages_in_order(chain, monkeypatch):
    lib, torch, app, hand, plain, values, cur, moved = chain
    from crychic_renderer_amd import renderer
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        for subset in SUBSETS:
            set_switches(app, subset, values)
            del rec.calls[:]
            app.Draw()
            assert rec.calls == LIGHTING + [name for s in subset for name in CALLS[s]], (subset, rec.calls)
        torch.cuda.synchronize()
    finally:
        set_switches(app, (), values)


def test_a_strip_or_a_shared_draw_is_refused_before_anything_is_issued(chain, monkeypatch):
    lib, torch, app, hand, plain, values, cur, moved = chain
    from crychic_renderer_amd import renderer
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        for subset in [(s,) for s in SWITCHES] + [SWITCHES]:
            set_switches(app, subset, values)
            del rec.calls[:]
            for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
                with pytest.raises(lib.CrychicError):
                    app.Draw(**kw)
            assert rec.calls == [], (subset, rec.calls)
            app.Draw(row0=0, rows=96)                           # the whole frame, spelled out
            assert rec.calls == LIGHTING + [name for s in subset for name in CALLS[s]], (subset, rec.calls)
    finally:
        set_switches(app, (), values)
    del rec.calls[:]
    app.Draw(row0=0, rows=48)                                   # without them a strip is a strip
    torch.cuda.synchronize()
    assert rec.calls == LIGHTING


def test_final_frame_is_the_last_set_stages_buffer(chain):
    lib, torch, app, hand, plain, values, cur, moved = chain
    try:
        for subset in SUBSETS:
            set_switches(app, subset, values)
            app.Draw()
            last = [s for s in subset if s != "fog"]
            want = getattr(app, BUFFER[last[-1]]) if last else app.mBackBuffer
            assert want is not None and app.final_frame() is want, subset
        torch.cuda.synchronize()
    finally:
        set_switches(app, (), values)
