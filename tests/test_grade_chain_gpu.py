"""The colour grade as Crychic.Draw chains it, between the bloom and the anti-aliasing: behind each possible nearest stage in front
(none, the fog alone, the bloom, the upsampling at the display's size), with the anti-aliasing behind it reading mBackBufferGrade; the
library calls by name with the switch set and unset; what colourGrade takes; the refusals; and where the finished frame is."""
import numpy as np
import pytest

import bloom_lib
import grade_lib as gl
from recorder_lib import Recorder

pytestmark = pytest.mark.gpu

W, H, SD = 128, 96, 256
LIGHTING = ["crychic_draw_hot_path_point_shadows"]
GRADE = dict(slope=(1.2, 1.0, 0.8), offset=(0.03, 0.0, -0.02), power=(0.9, 1.0, 1.2), saturation=1.3)


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


SWITCHES = ("fog", "temporalUpscale", "bloom", "colourGrade", "antiAliasing")


def clear(app):
    for s in SWITCHES:
        setattr(app, s, None)


def host_table(lib, params, N=33):
    import ctypes as C
    lut = np.zeros((N, N, N, 4), np.uint8)
    q = lib.GradeParams.default(**params)
    lib.check(lib.lib.crychic_grade_build_lut(C.byref(q), N, lut.ctypes.data, lut.nbytes))
    return lut


@pytest.mark.parametrize("front", ["none", "fog", "bloom", "temporalUpscale"])
def test_the_stage_behind_each_stage_in_front_and_the_anti_aliasing_behind_it(chain, front):
    lib, torch, app, hand = chain
    table = host_table(lib, GRADE)
    try:
        clear(app)
        app.colourGrade = lib.GradeParams.default(**GRADE)
        app.antiAliasing = True
        if front == "fog":
            app.fog = True
        elif front == "bloom":
            app.bloom = lib.BloomParams.default(**bloom_lib.SCENE_PARAMS)
        elif front == "temporalUpscale":
            app.temporalUpscale = (2 * W, 2 * H)
        app.Draw()
        torch.cuda.synchronize()
        src = {"none": app.mBackBuffer, "fog": app.mBackBuffer, "bloom": app.mBackBufferBloom, "temporalUpscale": app.mBackBufferUpscaled}[front]
        if front == "temporalUpscale":
            assert tuple(src.shape) == (2 * H, 2 * W, 4)
        if front == "fog":
            hand.Draw()
            torch.cuda.synchronize()
            assert not torch.equal(src, hand.mBackBuffer), "the fog did not run in front of the grade"
        ref = gl.checker(src.cpu().numpy(), table)
        assert tuple(app.mBackBufferGrade.shape) == tuple(src.shape)
        assert np.array_equal(app.mBackBufferGrade.cpu().numpy(), ref), "mBackBufferGrade is not the checker's grade of the stage in front"
        assert not np.array_equal(ref, src.cpu().numpy()), "the grade changes nothing on this scene: the test shows nothing"
        # the anti-aliasing behind it read the graded frame
        want = hand.antialias(src=app.mBackBufferGrade.clone(), out=torch.zeros_like(app.mBackBufferGrade))
        torch.cuda.synchronize()
        assert torch.equal(app.mBackBufferAA, want), "the anti-aliasing did not read mBackBufferGrade"
        assert app.final_frame() is app.mBackBufferAA
        app.antiAliasing = None
        assert app.final_frame() is app.mBackBufferGrade
    finally:
        clear(app)


def test_library_calls(chain, monkeypatch):
    lib, torch, app, hand = chain
    from crychic_renderer_amd import renderer
    clear(app)
    app.colourGrade = lib.GradeParams.default(**GRADE)           # builds and uploads here, not in Draw()
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_grade"], rec.calls
        app.bloom, app.antiAliasing = True, True
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_bloom_workspace_bytes", "crychic_bloom", "crychic_grade", "crychic_antialias"], rec.calls
        # unset: exactly the calls of a Draw() that never heard of the grade
        app.colourGrade = None
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_bloom_workspace_bytes", "crychic_bloom", "crychic_antialias"], rec.calls
        app.bloom = app.antiAliasing = None
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
    app.colourGrade = gl.identity_lut(16)
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError, match="colourGrade is set"):
                app.Draw(**kw)
        app.fog = True                                           # every earlier message stays: colourGrade is named last
        with pytest.raises(lib.CrychicError, match="fog is set"):
            app.Draw(row0=0, rows=48)
        assert rec.calls == []
    finally:
        clear(app)
    for bad in (np.zeros((3, 3, 4), np.uint8), np.zeros((3, 3, 3, 3), np.uint8), np.zeros((1, 1, 1, 4), np.uint8), np.zeros((34, 34, 34, 4), np.uint8),
                np.zeros((3, 3, 3, 4), np.float32), np.zeros((3, 4, 3, 4), np.uint8)):
        with pytest.raises(lib.CrychicError):
            app.colourGrade = bad
        assert app.colourGrade is None and not app._post
    with pytest.raises(lib.CrychicError):
        app.colourGrade = lib.GradeParams.default(saturation=9.0)
    with pytest.raises(lib.CrychicError):
        app.colourGrade = "/nonexistent/look.cube"
    with pytest.raises(lib.CrychicError):
        app.colour_grade()                                       # no table
    assert rec.calls == ["crychic_grade_build_lut", "crychic_load_cube_lut"], rec.calls


def test_what_colour_grade_takes(chain, tmp_path):
    """A table, a GradeParams and a .cube file of one look leave the same frame; colour_grade by hand, in place and into a buffer."""
    lib, torch, app, hand = chain
    table = host_table(lib, GRADE)
    path = gl.write_cube(tmp_path / "look.cube", table)
    hand.Draw()
    torch.cuda.synchronize()
    ref = gl.checker(hand.mBackBuffer.cpu().numpy(), table)
    try:
        for value in (lib.GradeParams.default(**GRADE), table, torch.from_numpy(table), str(path), path):
            clear(app)
            app.colourGrade = value
            assert tuple(app.mGradeLut.shape) == (33, 33, 33, 4) and np.array_equal(app.mGradeLut.cpu().numpy(), table)
            app.Draw()
            torch.cuda.synchronize()
            assert np.array_equal(app.final_frame().cpu().numpy(), ref), type(value)
    finally:
        clear(app)
    out = hand.colour_grade(lut=table)
    assert out is hand.mBackBufferGrade and np.array_equal(out.cpu().numpy(), ref)
    small = gl.corpus_lut(5)
    top = hand.colour_grade(lut=small, out=torch.full_like(hand.mBackBuffer, gl.GUARD), row0=1, rows=3).cpu().numpy()
    want = np.full_like(ref, gl.GUARD)
    want[1:4] = gl.checker(hand.mBackBuffer.cpu().numpy(), small)[1:4]
    assert np.array_equal(top, want)
    frame = hand.mBackBuffer.clone()
    assert hand.colour_grade(src=frame, out=frame, lut=table) is frame and np.array_equal(frame.cpu().numpy(), ref)
    assert not hand._post and hand.colourGrade is None
