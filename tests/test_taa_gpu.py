"""crychic_taa on the device: the kernel against the checker (tests/taa_ref) byte for byte in both outputs on the corpus of the CPU
tier, behind guard bytes and on misaligned planes; a five-frame sequence with a moving camera; the known answers; row ranges; and the
pass behind Crychic.Draw -- alone, with the fog in front, with the depth of field, the bloom and the anti-aliasing behind, switched
off, on a strip, and replayed from a graph."""
import ctypes as C

import numpy as np
import pytest

import taa_lib as ta
from post_pass_lib import dev      # noqa: F401 -- the module's fixture
from recorder_lib import Recorder

pytestmark = pytest.mark.gpu


def test_device_equals_checker(dev):
    for i, case in enumerate(ta.corpus()):
        ref_out, ref_hist, _ = ta.expected(case)
        out, hist = ta.run_device(dev, case, misalign=(0, 4, 12, 8)[i % 4])
        assert np.array_equal(out, ref_out), "%s: %d bytes of out differ" % (case.name, int((out != ref_out).sum()))
        assert np.array_equal(hist, ref_hist), "%s: %d words of history_out differ" % (case.name, int((hist != ref_hist).sum()))


def test_five_frames_with_a_moving_camera(dev):
    """The 70 x 38 synthetic scene under a camera that strafes, turns and dollies, jittered: after every frame `out` and both history
    planes equal the checker's."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import scene
    W, H = 70, 38
    rng = np.random.default_rng(38)
    cams = [ta.moved_camera(W, H), ta.moved_camera(W, H, dx=0.02), ta.moved_camera(W, H, dx=0.3, yaw=0.01), ta.moved_camera(W, H, dx=0.3, dz=0.8, yaw=0.05),
            ta.moved_camera(W, H, dx=0.3, dz=0.8, yaw=0.05)]
    hist_dev, hist_ref, prev, seen = None, None, None, 0
    for k, cam in enumerate(cams):
        consts = scene.Constants(W, H, 64, cam=cam, jitter=ta.jitter(k))
        depth = scene._camera_planes(consts, "cpu")["depth"].numpy().view(np.uint32)
        img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        img[..., :3] = (img[..., :3] >> 3) + (depth[..., None] >> 17).astype(np.uint8)      # the scene's shapes with a little noise
        cur = ta.camera_matrices(W, H, cam=cam)[0]
        ivp = np.array(consts.pass_cb.InvViewProj[:], np.float32)
        case_ref = ta.Case("frame%d" % k, ivp, cur, cur if prev is None else prev, depth, img, hist_ref, flags=ta.RESET if k == 0 else 0)
        case_dev = ta.Case("frame%d" % k, ivp, cur, cur if prev is None else prev, depth, img, hist_dev, flags=ta.RESET if k == 0 else 0)
        out_ref, new_ref, branch = ta.checker(case_ref)
        out_dev, new_dev = ta.run_device(dev, case_dev, misalign=4 * (k % 2))
        assert np.array_equal(out_dev, out_ref) and np.array_equal(new_dev, new_ref), k
        assert hist_dev is None or np.array_equal(hist_dev, hist_ref), "the history read changed"
        seen += int(((branch & ta.B_HISTORY) != 0).sum())
        hist_dev, hist_ref, prev = new_dev, new_ref, cur
    assert seen > 2 * W * H


def test_known_answers(dev):
    from test_taa_host import answers
    answers(lambda c: ta.run_device(dev, c))
    answers(lambda c: ta.run_device(dev, c, misalign=12))


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 189, 190)])
def test_row_ranges_stitch_to_the_whole_frame(dev, split):
    from test_taa_host import tall_case
    case = tall_case("dolly")
    whole_out, whole_hist, _ = ta.checker(case)
    s_out, s_hist = np.full_like(whole_out, ta.GUARD), np.full_like(whole_hist, ta.GUARD * 257)
    for row0, end in zip(split[:-1], split[1:]):
        out, hist = ta.run_device(dev, case, row0=row0, rows=end - row0, misalign=4 if row0 else 0)
        for plane, guard in ((out, ta.GUARD), (hist, ta.GUARD * 257)):
            assert (plane[:row0] == guard).all() and (plane[end:] == guard).all(), "rows outside the range were written"
        s_out[row0:end], s_hist[row0:end] = out[row0:end], hist[row0:end]
    assert np.array_equal(s_out, whole_out) and np.array_equal(s_hist, whole_hist)
    out, hist = ta.run_device(dev, case, row0=190, rows=0)
    assert (out == ta.GUARD).all() and (hist == ta.GUARD * 257).all()


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    W, H = 64, 32
    a = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((H, W, 4), ta.GUARD, dtype=torch.uint8, device=ctx.device)
    h0 = torch.zeros((H, W, 4), dtype=torch.int16, device=ctx.device)
    h1 = torch.full((H, W, 4), 0x5A5A, dtype=torch.int16, device=ctx.device)
    d = torch.zeros((H, W), dtype=torch.int32, device=ctx.device)
    pa, pb, p0, p1, pd = (C.c_void_p(t.data_ptr()) for t in (a, b, h0, h1, d))
    cb = lib.PassConstants()
    cb.InvViewProj[:] = list(ta.IDENTITY)
    eye = (C.c_float * 16)(*ta.IDENTITY)
    f = lib.lib.crychic_taa
    err = lib.lib.crychic_last_error
    assert f(ctx.handle, C.byref(cb), eye, eye, pd, pa, p0, p1, C.c_void_p(a.data_ptr() + 4), W, H, 0, H, None, None) == -1 and "overlap" in err().decode()
    assert f(ctx.handle, C.byref(cb), eye, eye, pd, pa, p0, p0, pb, W, H, 0, H, None, None) == -1 and "history planes overlap" in err().decode()
    assert f(ctx.handle, C.byref(cb), eye, eye, pd, pa, None, p1, pb, W, H, 0, H, None, None) == -1 and "null argument" in err().decode()
    assert f(ctx.handle, C.byref(cb), eye, eye, pd, pa, p0, p1, pb, W, H, 1, H, None, None) == -1
    bad = lib.TaaParams.default(blend=300)
    assert f(ctx.handle, C.byref(cb), eye, eye, pd, pa, p0, p1, pb, W, H, 0, H, C.byref(bad), None) == -1 and "blend" in err().decode()
    torch.cuda.synchronize()
    assert bool((b == ta.GUARD).all()) and bool((h1 == 0x5A5A).all()), "a refused call wrote"


def test_one_captured_call_replays_to_the_same_bytes(dev):
    lib, ctx, torch = dev
    case = {c.name: c for c in ta.corpus()}["smooth_dolly"]
    ref_out, ref_hist, _ = ta.expected(case)
    H, W = case.H, case.W
    src = torch.from_numpy(case.img.copy()).to(ctx.device)
    depth = torch.from_numpy(case.depth.view(np.int32).copy()).to(ctx.device)
    hin = torch.from_numpy(case.hist.view(np.int16).copy()).to(ctx.device)
    out, hout = torch.zeros_like(src), torch.zeros_like(hin)
    pcb = case.pass_constants(lib)
    p = lib.TaaParams.default(blend=case.blend, flags=case.flags)
    cur, prev = (C.c_float * 16)(*case.cur), (C.c_float * 16)(*case.prev)

    def call():
        s = torch.cuda.current_stream(ctx.device)
        lib.check(lib.lib.crychic_taa(ctx.handle, C.byref(pcb), cur, prev, C.c_void_p(depth.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(hin.data_ptr()),
                                      C.c_void_p(hout.data_ptr()), C.c_void_p(out.data_ptr()), W, H, 0, H, C.byref(p), C.c_void_p(s.cuda_stream)))
    call()                              # before the capture: the code object loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        out.zero_()
        hout.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref_out) and np.array_equal(hout.cpu().numpy().view(np.uint16), ref_hist)


# ---- behind Crychic.Draw ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def app_frame(dev):
    """A Crychic over the 128 x 96 synthetic scene and the frame Draw() gives without the pass."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    W, H, SD = 128, 96, 256
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 3, 3, LIGHT_SKY
    assert app.temporalAA is None
    app.Draw()
    torch.cuda.synchronize()
    return app, app.mBackBuffer.cpu().numpy().copy(), planes


def case_of(app, planes, img, hist, cur, prev, reset, blend=ta.DEFAULT_BLEND):
    return ta.Case("draw", np.array(app.mMainPassCB.InvViewProj[:], np.float32), cur, prev, planes["depth"].cpu().numpy().view(np.uint32), img, hist, blend,
                   ta.RESET if reset else 0)


def history(app):
    return app.mTaaHistory[0].cpu().numpy().view(np.uint16)


def test_draw_with_temporal_aa(dev, app_frame):
    """Draw() with temporalAA alone equals the chain issued by hand: a RESET frame first, then the history of the frame before through
    the matrices of set_frame_view_proj; a TaaParams reaches the pass; turning the switch off and on again is a RESET frame."""
    lib, ctx, torch = dev
    app, plain, planes = app_frame
    cur = np.array(app.mMainPassCB.ViewProj[:], np.float32)
    moved = ta.camera_matrices(128, 96, cam=ta.moved_camera(128, 96, dx=0.05))[0]
    app.temporalAA = True
    try:
        app.Draw()                                              # no set_frame_view_proj yet: the constants' own ViewProj, a RESET frame
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "mBackBuffer stays the frame without the pass"
        assert np.array_equal(app.mBackBufferTAA.cpu().numpy(), plain) and np.array_equal(history(app), plain.astype(np.uint16) * 256)
        h0 = history(app).copy()
        app.set_frame_view_proj(moved)                          # the "previous" frame's
        app.set_frame_view_proj(cur)
        app.Draw()
        torch.cuda.synchronize()
        out, h1, branch = ta.checker(case_of(app, planes, plain, h0, cur, moved, False))
        assert (branch & ta.B_FX).any() and not np.array_equal(out, plain)
        assert np.array_equal(app.mBackBufferTAA.cpu().numpy(), out) and np.array_equal(history(app), h1)
        app.temporalAA = lib.TaaParams.default(blend=200)       # parameters while it is on: no reset
        app.set_frame_view_proj(cur)
        app.Draw()
        torch.cuda.synchronize()
        out, h2, _ = ta.checker(case_of(app, planes, plain, h1, cur, cur, False, blend=200))
        assert np.array_equal(app.mBackBufferTAA.cpu().numpy(), out) and np.array_equal(history(app), h2)
        app.temporalAA = None
        app.temporalAA = True                                   # off and on again: a RESET frame
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferTAA.cpu().numpy(), plain) and np.array_equal(history(app), plain.astype(np.uint16) * 256)
    finally:
        app.temporalAA = None


def test_fog_in_front_and_the_other_passes_behind(dev, app_frame):
    """lighting -> fog -> temporal anti-aliasing -> depth of field -> bloom -> anti-aliasing: every buffer equals its checker over the
    one before."""
    lib, ctx, torch = dev
    import bloom_lib
    import dof_lib
    import fog_lib
    import post_aa_lib as aa
    app, plain, planes = app_frame
    depth = planes["depth"].cpu().numpy().view(np.uint32)
    fogged, _ = fog_lib.checker(fog_lib.Frame.from_pass_cb(app.mMainPassCB, depth, planes["shadow"].cpu().numpy().view(np.uint32)), plain)
    cur = np.array(app.mMainPassCB.ViewProj[:], np.float32)
    moved = ta.camera_matrices(128, 96, cam=ta.moved_camera(128, 96, dx=-0.04, yaw=0.002))[0]
    app.fog, app.temporalAA = True, True
    try:
        app.Draw()                                              # the RESET frame of the fogged sequence
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), fogged) and np.array_equal(app.mBackBufferTAA.cpu().numpy(), fogged)
        h0 = history(app).copy()
        app.set_frame_view_proj(moved)
        app.set_frame_view_proj(cur)
        app.depthOfField, app.bloom, app.antiAliasing = True, True, True
        app.Draw()
        torch.cuda.synchronize()
        resolved, h1, _ = ta.checker(case_of(app, planes, fogged, h0, cur, moved, False))
        assert not np.array_equal(resolved, fogged)
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), fogged)
        assert np.array_equal(app.mBackBufferTAA.cpu().numpy(), resolved) and np.array_equal(history(app), h1)
        blurred, _ = dof_lib.checker(dof_lib.Frame.from_pass_cb(app.mMainPassCB, depth), resolved)
        assert np.array_equal(app.mBackBufferDoF.cpu().numpy(), blurred), "the depth of field did not read mBackBufferTAA"
        bloomed = bloom_lib.checker(blurred)[0]
        assert np.array_equal(app.mBackBufferBloom.cpu().numpy(), bloomed)
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), aa.checker(bloomed)[0])
        # without the depth of field and the bloom the anti-aliasing reads mBackBufferTAA
        app.depthOfField, app.bloom = None, None
        app.set_frame_view_proj(cur)
        app.Draw()
        torch.cuda.synchronize()
        resolved2, _, _ = ta.checker(case_of(app, planes, fogged, h1, cur, cur, False))
        assert np.array_equal(app.mBackBufferTAA.cpu().numpy(), resolved2)
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), aa.checker(resolved2)[0])
        assert app.fog is True and app.temporalAA is True and app.antiAliasing is True
    finally:
        app.fog, app.temporalAA, app.depthOfField, app.bloom, app.antiAliasing = None, None, None, None, None


def test_switch_off_is_the_frame_and_the_calls_of_before(dev, app_frame, monkeypatch):
    lib, ctx, torch = dev
    from crychic_renderer_amd import renderer
    app, plain, planes = app_frame
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    assert app.temporalAA is None and not app._post
    app.Draw()
    torch.cuda.synchronize()
    assert rec.calls == ["crychic_draw_hot_path_point_shadows"], rec.calls
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
    del rec.calls[:]
    app.temporalAA = True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert rec.calls == ["crychic_draw_hot_path_point_shadows", "crychic_taa"], rec.calls
    finally:
        app.temporalAA = None
    del rec.calls[:]
    app.Draw()
    torch.cuda.synchronize()
    assert rec.calls == ["crychic_draw_hot_path_point_shadows"] and np.array_equal(app.mBackBuffer.cpu().numpy(), plain)


def test_strip_or_shared_draw_raises(dev, app_frame):
    lib, ctx, torch = dev
    app, plain, planes = app_frame
    app.temporalAA = True
    try:
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError):
                app.Draw(**kw)
        app.Draw(row0=0, rows=96)           # the whole frame, spelled out
    finally:
        app.temporalAA = None
    app.Draw(row0=0, rows=48)               # without it a strip is a strip
    torch.cuda.synchronize()
