"""The temporal upsampling as Crychic.Draw chains it,

    lighting -> ssr -> fog (in place) -> temporal upsampling -> bloom -> anti-aliasing,

over every subset of the five switches that holds the upsampling: the bytes of every buffer against the same passes issued by hand on
a second object, the library calls by name, the shape of the finished frame, the four refusals, and the switch off."""
import numpy as np
import pytest

import bloom_lib
import motion_blur_lib as mbl
import taa_upscale_lib as tu
from recorder_lib import Recorder

pytestmark = pytest.mark.gpu

SWITCHES = ("ssr", "fog", "temporalUpscale", "bloom", "antiAliasing")          # in the chain's order
BUFFER = dict(ssr="mBackBufferSSR", temporalUpscale="mBackBufferUpscaled", bloom="mBackBufferBloom", antiAliasing="mBackBufferAA")
SUBSETS = [s for s in (tuple(s for k, s in enumerate(SWITCHES) if mask >> k & 1) for mask in range(32)) if "temporalUpscale" in s]
LIGHTING = ["crychic_draw_hot_path_point_shadows"]
CALLS = dict(ssr=["crychic_ssr"], fog=["crychic_fog"], temporalUpscale=["crychic_taa_upscale"], bloom=["crychic_bloom_workspace_bytes", "crychic_bloom"],
             antiAliasing=["crychic_antialias"])
W, H, SD = 128, 96, 256
WO, HO = 192, 144


@pytest.fixture(scope="module")
def chain(built_lib):
    """Two Crychic over the planes of one 128 x 96 synthetic scene -- `app` for Draw(), `hand` whose switches are never set --, the
    frame without a pass, the value of each switch and the two cameras."""
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
    values["temporalUpscale"] = (WO, HO)
    cur = np.array(app.mMainPassCB.ViewProj[:], np.float32)
    moved = mbl.camera_matrices(W, H, cam=mbl.moved_camera(W, H, dx=-0.3, yaw=0.02))[0]
    jit = tu.halton(1)
    for a in apps:                                              # the camera has moved between the two frames
        a.set_frame_view_proj(moved)
        a.set_frame_view_proj(cur, jitter=jit)
    yield lib, torch, app, hand, plain, values, cur, moved, jit
    ctx.close()


def set_switches(app, subset, values):
    for s in SWITCHES:
        setattr(app, s, None)
    for s in subset:
        setattr(app, s, values[s])


def issue_by_hand(hand, subset, values, cur, prev, jit, reset):
    """A frame and the stages of `subset` through the public pass methods, each from what the stage in front returned."""
    hand.Draw()
    frame = hand.mBackBuffer
    if "ssr" in subset:
        frame = hand.screen_space_reflections(src=frame)
    if "fog" in subset:
        frame = hand.apply_fog(src=frame)
    frame = hand.temporal_upscale(cur, prev, jit, (WO, HO), src=frame, reset=reset)
    if "bloom" in subset:
        frame = hand.apply_bloom(src=frame, params=values["bloom"])
    if "antiAliasing" in subset:
        frame = hand.antialias(src=frame)
    return frame


def test_every_subset_leaves_the_bytes_of_the_passes_issued_by_hand(chain):
    lib, torch, app, hand, plain, values, cur, moved, jit = chain
    try:
        for subset in SUBSETS:
            set_switches(app, subset, values)                   # from cleared: the first frame is a RESET frame
            for frame in range(2):
                app.Draw()
                last = issue_by_hand(hand, subset, values, cur, moved, jit, reset=frame == 0)
                torch.cuda.synchronize()
                where = "%s, frame %d" % ("+".join(subset), frame)
                src = app.mBackBufferSSR if "ssr" in subset else app.mBackBuffer
                for s in (s for s in subset if s != "fog"):
                    got, want = getattr(app, BUFFER[s]), getattr(hand, BUFFER[s])
                    assert torch.equal(got, want), "%s: %s" % (where, BUFFER[s])
                    assert tuple(got.shape) == ((H, W, 4) if s == "ssr" else (HO, WO, 4)), "%s: %s" % (where, BUFFER[s])
                    if s != "ssr":
                        assert got.shape != src.shape or not torch.equal(got, src), "%s: %s changed nothing" % (where, s)
                    src = got
                assert torch.equal(app.mTaaUpscaleHistory[0], hand.mTaaUpscaleHistory[0]), where
                assert last is getattr(hand, BUFFER[[s for s in subset if s != "fog"][-1]]), where
                assert app.final_frame() is getattr(app, BUFFER[[s for s in subset if s != "fog"][-1]]) and tuple(app.final_frame().shape) == (HO, WO, 4), where
            assert not hand._post
    finally:
        set_switches(app, (), values)


def test_the_second_frame_is_the_checkers(chain):
    """Draw() with the upsampling alone and its parameters: a RESET frame, then the checker's frame over the first one's history
    through the matrices and the jitter of set_frame_view_proj."""
    lib, torch, app, hand, plain, values, cur, moved, jit = chain
    depth = app.mDepthStencilBuffer.cpu().numpy().view(np.uint32)
    ivp = np.array(app.mMainPassCB.InvViewProj[:], np.float32)
    img = plain.cpu().numpy()
    try:
        app.temporalUpscale = (WO, HO, lib.TaaUpscaleParams.default(blend=200))
        app.Draw()
        out0, h0, _ = tu.checker(tu.Case("draw0", ivp, cur, moved, jit, depth, img, (WO, HO), None, blend=200, flags=tu.RESET))
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferUpscaled.cpu().numpy(), out0) and np.array_equal(app.mTaaUpscaleHistory[0].cpu().numpy().view(np.uint16), h0)
        app.Draw()
        out1, h1, branch = tu.checker(tu.Case("draw1", ivp, cur, moved, jit, depth, img, (WO, HO), h0, blend=200))
        torch.cuda.synchronize()
        assert (branch & tu.B_FX).any() and not np.array_equal(out1, out0)
        assert np.array_equal(app.mBackBufferUpscaled.cpu().numpy(), out1) and np.array_equal(app.mTaaUpscaleHistory[0].cpu().numpy().view(np.uint16), h1)
        app.temporalUpscale = None
        app.temporalUpscale = (WO, HO)                          # off and on again: a RESET frame
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mTaaUpscaleHistory[0].cpu().numpy().view(np.uint16), h0)
    finally:
        set_switches(app, (), values)


def test_every_subset_issues_the_calls_of_its_stages_in_order(chain, monkeypatch):
    lib, torch, app, hand, plain, values, cur, moved, jit = chain
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


def test_the_four_refusals_issue_nothing(chain, monkeypatch):
    """A strip or a shared draw, and the upsampling together with the temporal anti-aliasing, the depth of field or the motion blur."""
    lib, torch, app, hand, plain, values, cur, moved, jit = chain
    from crychic_renderer_amd import renderer
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        app.temporalUpscale = (WO, HO)
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError, match="temporalUpscale is set"):
                app.Draw(**kw)
        for other in ("temporalAA", "depthOfField", "motionBlur"):
            setattr(app, other, True)
            with pytest.raises(lib.CrychicError, match="temporalUpscale and %s are both set" % other):
                app.Draw()
            setattr(app, other, None)
        app.temporalUpscale = (WO, HO, 7)
        with pytest.raises(lib.CrychicError, match="TaaUpscaleParams"):
            app.Draw()
        assert rec.calls == [], rec.calls
        app.temporalUpscale = (4 * W + 1, HO)                   # the library's own refusal, behind the lighting frame
        with pytest.raises(lib.CrychicError, match="ratio"):
            app.Draw()
        torch.cuda.synchronize()
    finally:
        for other in ("temporalAA", "depthOfField", "motionBlur"):
            setattr(app, other, None)
        set_switches(app, (), values)


def test_switch_off_is_the_frame_and_the_calls_of_before(chain, monkeypatch):
    lib, torch, app, hand, plain, values, cur, moved, jit = chain
    from crychic_renderer_amd import renderer
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    assert app.temporalUpscale is None and not app._post
    app.Draw()
    torch.cuda.synchronize()
    assert rec.calls == LIGHTING and torch.equal(app.mBackBuffer, plain) and app.final_frame() is app.mBackBuffer
    app.temporalUpscale = (WO, HO)
    try:
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + CALLS["temporalUpscale"]
    finally:
        app.temporalUpscale = None
    del rec.calls[:]
    app.Draw(row0=0, rows=48)                                   # without it a strip is a strip
    app.Draw()
    torch.cuda.synchronize()
    assert rec.calls == LIGHTING * 2 and torch.equal(app.mBackBuffer, plain)
