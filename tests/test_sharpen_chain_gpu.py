"""The sharpening as Crychic.Draw chains it, directly behind the temporal stage and in front of the depth of field,

    lighting -> ... -> temporalAA | temporalUpscale -> sharpening -> depthOfField -> ... -> antiAliasing:

with the switch set alone and behind each temporal stage, with and without a stage behind it (the depth of field; behind the
upsampling, which does not go with it, the anti-aliasing), the bytes of every buffer against the same passes issued by hand on a second
object and against the checker; the library calls by name and in order; final_frame(); the switch unset; and the refusals."""
import numpy as np
import pytest

import sharpen_lib as sl
from recorder_lib import Recorder

pytestmark = pytest.mark.gpu

W, H, SD = 128, 96, 256
WO, HO = 192, 144
LIGHTING = ["crychic_draw_hot_path_point_shadows"]
SWITCHES = ("fog", "temporalAA", "temporalUpscale", "sharpening", "depthOfField", "bloom", "antiAliasing")
CASES = [(front, behind) for front in (None, "temporalAA", "temporalUpscale") for behind in (None, "depthOfField", "antiAliasing")
         if not (front == "temporalUpscale" and behind == "depthOfField")]


@pytest.fixture(scope="module")
def chain(built_lib):
    """Two Crychic over the planes of one 128 x 96 synthetic scene: `app` for Draw(), `hand` whose switches are never set."""
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, scene
    ctx = Context(0)
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    apps = []
    for _ in range(2):
        a = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
        a.load_scene(planes)
        a.blurCount, a.numDirLights, a.flags = 3, 3, LIGHT_SKY
        apps.append(a)
    yield built_lib, torch, apps[0], apps[1]
    ctx.close()


def clear(app):
    for s in SWITCHES:
        setattr(app, s, None)


@pytest.mark.parametrize("front,behind", CASES)
def test_draw_leaves_the_bytes_of_the_passes_issued_by_hand(chain, front, behind):
    lib, torch, app, hand = chain
    strong = lib.SharpenParams.default(strength=256, limit=3584)
    cur = tuple(app.mMainPassCB.ViewProj)                       # set_frame_view_proj is never called: a still camera, no jitter
    try:
        clear(app)
        app.sharpening = strong
        if front == "temporalAA":
            app.temporalAA = True
        elif front == "temporalUpscale":
            app.temporalUpscale = (WO, HO)
        if behind:
            setattr(app, behind, True)
        for frame in range(2):                                  # from cleared: the first frame is a RESET frame
            app.Draw()
            hand.Draw()
            src = hand.mBackBuffer
            if front == "temporalAA":
                src = hand.temporal_aa(cur, cur, src=src, reset=frame == 0)
            elif front == "temporalUpscale":
                src = hand.temporal_upscale(cur, cur, (0.0, 0.0), (WO, HO), src=src, reset=frame == 0)
            sharp = hand.sharpen_frame(src=src, params=strong)
            last = sharp
            if behind == "depthOfField":
                last = hand.depth_of_field(src=sharp)
            elif behind == "antiAliasing":
                last = hand.antialias(src=sharp)
            torch.cuda.synchronize()
            where = "%s -> sharpening -> %s, frame %d" % (front, behind, frame)
            read = {None: app.mBackBuffer, "temporalAA": app.mBackBufferTAA, "temporalUpscale": app.mBackBufferUpscaled}[front]
            assert torch.equal(read, src), where
            assert tuple(app.mBackBufferSharp.shape) == ((HO, WO, 4) if front == "temporalUpscale" else (H, W, 4)), where
            assert torch.equal(app.mBackBufferSharp, sharp), where
            ref = sl.checker(read.cpu().numpy(), 256, 3584)
            assert np.array_equal(app.mBackBufferSharp.cpu().numpy(), ref), where + ": not the checker's frame of the stage in front"
            assert not np.array_equal(ref, read.cpu().numpy()), where + ": the pass changes nothing on this scene"
            if behind:
                buffer = {"depthOfField": "mBackBufferDoF", "antiAliasing": "mBackBufferAA"}[behind]
                assert torch.equal(getattr(app, buffer), last), where + ": the stage behind did not read mBackBufferSharp"
                assert app.final_frame() is getattr(app, buffer), where
            else:
                assert app.final_frame() is app.mBackBufferSharp, where
        assert not hand._post
    finally:
        clear(app)


def test_default_parameters(chain):
    """sharpening = True is crychic_sharpen_default_params."""
    lib, torch, app, hand = chain
    d = lib.SharpenParams.default()
    try:
        clear(app)
        app.sharpening = True
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferSharp.cpu().numpy(), sl.checker(app.mBackBuffer.cpu().numpy(), d.strength, d.limit))
    finally:
        clear(app)


def test_library_calls(chain, monkeypatch):
    lib, torch, app, hand = chain
    from crychic_renderer_amd import renderer
    clear(app)
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        app.sharpening = True
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_sharpen"], rec.calls
        app.fog, app.temporalAA, app.depthOfField, app.bloom, app.antiAliasing = True, True, True, True, True
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_fog", "crychic_taa", "crychic_sharpen", "crychic_dof", "crychic_bloom_workspace_bytes", "crychic_bloom",
                                        "crychic_antialias"], rec.calls
        # unset: exactly the calls of a Draw() that never heard of the sharpening
        app.sharpening = None
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_fog", "crychic_taa", "crychic_dof", "crychic_bloom_workspace_bytes", "crychic_bloom", "crychic_antialias"], rec.calls
        assert app.final_frame() is app.mBackBufferAA
        clear(app)
        app.temporalUpscale, app.sharpening, app.bloom = (WO, HO), True, True
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_taa_upscale", "crychic_sharpen", "crychic_bloom_workspace_bytes", "crychic_bloom"], rec.calls
        clear(app)
        assert not app._post
        del rec.calls[:]
        app.Draw()
        app.Draw(row0=0, rows=48)
        assert rec.calls == LIGHTING * 2, rec.calls
        torch.cuda.synchronize()
    finally:
        clear(app)


def test_refusals_issue_nothing(chain, monkeypatch):
    lib, torch, app, hand = chain
    from crychic_renderer_amd import renderer
    clear(app)
    app.sharpening = True
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError, match="sharpening is set"):
                app.Draw(**kw)
        for earlier in ("fog", "temporalAA", "antiAliasing", "bloom"):          # every earlier message stays: sharpening is named last
            setattr(app, earlier, True)
            with pytest.raises(lib.CrychicError, match="%s is set" % earlier):
                app.Draw(row0=0, rows=48)
            setattr(app, earlier, None)
        assert rec.calls == []
        app.sharpening = lib.SharpenParams.default(strength=300)
        with pytest.raises(lib.CrychicError, match="strength"):
            app.Draw()
        assert rec.calls == LIGHTING + ["crychic_sharpen"]
    finally:
        clear(app)
    with pytest.raises(lib.CrychicError):
        hand.sharpen_frame(src=hand.mBackBuffer, out=hand.mBackBuffer)          # in place
    torch.cuda.synchronize()


def test_sharpen_frame_by_hand(chain):
    """Row ranges into a caller's buffer, and a frame of another shape."""
    lib, torch, app, hand = chain
    hand.Draw()
    torch.cuda.synchronize()
    img = hand.mBackBuffer.cpu().numpy()
    p = lib.SharpenParams.default(strength=200)
    out = hand.sharpen_frame(out=torch.full_like(hand.mBackBuffer, sl.GUARD), row0=H - 3, rows=3, params=p).cpu().numpy()
    want = np.full_like(img, sl.GUARD)
    want[H - 3:] = sl.checker(img, 200, p.limit)[H - 3:]
    assert np.array_equal(out, want)
    other = torch.from_numpy(np.array(sl.frame(13, 17, "smooth"))).to(hand.mBackBuffer.device)
    got = hand.sharpen_frame(src=other, params=p)
    assert got is hand.mBackBufferSharp and np.array_equal(got.cpu().numpy(), sl.checker(sl.frame(13, 17, "smooth"), 200, p.limit))
    assert not hand._post and hand.sharpening is None
