"""crychic_taa_upscale on the device: the kernel against the checker (tests/taa_upscale_ref) byte for byte in both outputs on the corpus
of the CPU tier, behind guard bytes and on misaligned planes; a five-frame sequence with a moving camera and swapped histories; the
known answers, ratio 1 against Crychic.temporal_aa on the device among them; row ranges; refusals with a context; one captured call;
and the convergence orderings on the device's output."""
import ctypes as C

import numpy as np
import pytest

import taa_lib as ta
import taa_upscale_lib as tu
from post_pass_lib import dev      # noqa: F401 -- the module's fixture

pytestmark = pytest.mark.gpu


def test_device_equals_checker(dev):
    for i, case in enumerate(tu.corpus()):
        ref_out, ref_hist, _ = tu.expected(case)
        out, hist = tu.run_device(dev, case, misalign=(0, 4, 12, 8)[i % 4])
        assert np.array_equal(out, ref_out), "%s: %d bytes of out differ" % (case.name, int((out != ref_out).sum()))
        assert np.array_equal(hist, ref_hist), "%s: %d words of history_out differ" % (case.name, int((hist != ref_hist).sum()))


def test_five_frames_with_a_moving_camera(dev):
    """The 70 x 38 synthetic scene under a camera that strafes, turns and dollies, jittered, resolved at 105 x 60: after every frame
    `out` and both history planes equal the checker's."""
    from crychic_renderer_amd import scene
    W, H, Wo, Ho = 70, 38, 105, 60
    rng = np.random.default_rng(39)
    cams = [ta.moved_camera(W, H), ta.moved_camera(W, H, dx=0.02), ta.moved_camera(W, H, dx=0.3, yaw=0.01), ta.moved_camera(W, H, dx=0.3, dz=0.8, yaw=0.05),
            ta.moved_camera(W, H, dx=0.3, dz=0.8, yaw=0.05)]
    hist_dev, hist_ref, prev, seen = None, None, None, 0
    for k, cam in enumerate(cams):
        jit = tu.halton(k)
        consts = scene.Constants(W, H, 64, cam=cam, jitter=jit)
        depth = scene._camera_planes(consts, "cpu")["depth"].numpy().view(np.uint32)
        img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        img[..., :3] = (img[..., :3] >> 3) + (depth[..., None] >> 17).astype(np.uint8)      # the scene's shapes with a little noise
        cur = ta.camera_matrices(W, H, cam=cam)[0]
        ivp = np.array(consts.pass_cb.InvViewProj[:], np.float32)
        flags = tu.RESET if k == 0 else 0
        out_ref, new_ref, branch = tu.checker(tu.Case("frame%d" % k, ivp, cur, cur if prev is None else prev, jit, depth, img, (Wo, Ho), hist_ref, flags=flags))
        out_dev, new_dev = tu.run_device(dev, tu.Case("frame%d" % k, ivp, cur, cur if prev is None else prev, jit, depth, img, (Wo, Ho), hist_dev, flags=flags),
                                         misalign=4 * (k % 2))
        assert np.array_equal(out_dev, out_ref) and np.array_equal(new_dev, new_ref), k
        seen += int(((branch & tu.B_HISTORY) != 0).sum())
        hist_dev, hist_ref, prev = new_dev, new_ref, cur
    assert seen > 2 * Wo * Ho


def test_known_answers(dev):
    tu.answers(lambda c: tu.run_device(dev, c))
    tu.answers(lambda c: tu.run_device(dev, c, misalign=12))


def test_ratio_one_is_temporal_aa_on_the_device(dev):
    """Two frames under a moved camera through Crychic.temporal_aa and through Crychic.temporal_upscale at the frame's own size with
    zero jitter and the same blend: the same bytes in the frame and in the history."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    W, H, SD = 128, 96, 256
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 3, 3, LIGHT_SKY
    app.Draw()
    cur = np.array(app.mMainPassCB.ViewProj[:], np.float32)
    moved = ta.camera_matrices(W, H, cam=ta.moved_camera(W, H, dx=0.05, yaw=0.01))[0]
    for frame, prev in enumerate((cur, moved)):
        a = app.temporal_aa(cur, prev, reset=frame == 0, params=lib.TaaParams.default(blend=77))
        b = app.temporal_upscale(cur, prev, (0.0, 0.0), (W, H), reset=frame == 0, params=lib.TaaUpscaleParams.default(blend=77))
        torch.cuda.synchronize()
        assert b is app.mBackBufferUpscaled and torch.equal(a, b), frame
        assert torch.equal(app.mTaaHistory[0], app.mTaaUpscaleHistory[0]), frame
    assert not torch.equal(app.mBackBufferUpscaled, app.mBackBuffer), "the second frame blended a moved history"


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 189, 190)])
def test_row_ranges_stitch_to_the_whole_frame(dev, split):
    from test_taa_upscale_host import tall_case
    case = tall_case("dolly")
    whole_out, whole_hist, _ = tu.checker(case)
    s_out, s_hist = np.full_like(whole_out, tu.GUARD), np.full_like(whole_hist, tu.GUARD * 257)
    for row0, end in zip(split[:-1], split[1:]):
        out, hist = tu.run_device(dev, case, row0=row0, rows=end - row0, misalign=4 if row0 else 0)
        for plane, guard in ((out, tu.GUARD), (hist, tu.GUARD * 257)):
            assert (plane[:row0] == guard).all() and (plane[end:] == guard).all(), "rows outside the range were written"
        s_out[row0:end], s_hist[row0:end] = out[row0:end], hist[row0:end]
    assert np.array_equal(s_out, whole_out) and np.array_equal(s_hist, whole_hist)
    out, hist = tu.run_device(dev, case, row0=190, rows=0)
    assert (out == tu.GUARD).all() and (hist == tu.GUARD * 257).all()


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    Wi, Hi, Wo, Ho = 64, 32, 96, 48
    a = torch.zeros((Hi, Wi, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((Ho, Wo, 4), tu.GUARD, dtype=torch.uint8, device=ctx.device)
    h0 = torch.zeros((Ho, Wo, 4), dtype=torch.int16, device=ctx.device)
    h1 = torch.full((Ho, Wo, 4), 0x5A5A, dtype=torch.int16, device=ctx.device)
    d = torch.zeros((Hi, Wi), dtype=torch.int32, device=ctx.device)
    pa, pb, p0, p1, pd = (C.c_void_p(t.data_ptr()) for t in (a, b, h0, h1, d))
    cb = lib.PassConstants()
    cb.InvViewProj[:] = list(ta.IDENTITY)
    eye = (C.c_float * 16)(*ta.IDENTITY)
    f = lib.lib.crychic_taa_upscale
    err = lib.lib.crychic_last_error
    assert f(ctx.handle, C.byref(cb), eye, eye, 0.0, 0.0, pd, pa, Wi, Hi, p0, p1, C.c_void_p(a.data_ptr() + 4), Wo, Ho, 0, Ho, None, None) == -1 and "overlap" in err().decode()
    assert f(ctx.handle, C.byref(cb), eye, eye, 0.0, 0.0, pd, pa, Wi, Hi, p0, p0, pb, Wo, Ho, 0, Ho, None, None) == -1 and "history planes overlap" in err().decode()
    assert f(ctx.handle, C.byref(cb), eye, eye, 0.0, 0.0, pd, pa, Wi, Hi, None, p1, pb, Wo, Ho, 0, Ho, None, None) == -1 and "null argument" in err().decode()
    assert f(ctx.handle, C.byref(cb), eye, eye, 0.0, 0.0, pd, pa, Wi, Hi, p0, p1, pb, Wo, Ho, 1, Ho, None, None) == -1
    assert f(ctx.handle, C.byref(cb), eye, eye, 0.75, 0.0, pd, pa, Wi, Hi, p0, p1, pb, Wo, Ho, 0, Ho, None, None) == -1 and "jitter" in err().decode()
    assert f(ctx.handle, C.byref(cb), eye, eye, 0.0, 0.0, pd, pa, Wi, Hi, p0, p1, pb, 4 * Wi + 1, Ho, 0, Ho, None, None) == -1 and "ratio" in err().decode()
    bad = lib.TaaUpscaleParams.default(blend=300)
    assert f(ctx.handle, C.byref(cb), eye, eye, 0.0, 0.0, pd, pa, Wi, Hi, p0, p1, pb, Wo, Ho, 0, Ho, C.byref(bad), None) == -1 and "blend" in err().decode()
    torch.cuda.synchronize()
    assert bool((b == tu.GUARD).all()) and bool((h1 == 0x5A5A).all()), "a refused call wrote"


def test_one_captured_call_replays_to_the_same_bytes(dev):
    lib, ctx, torch = dev
    case = next(c for c in tu.corpus() if c.name.startswith("47x26_70x38") and c.jitter != (0.0, 0.0) and "dolly" in c.name and not c.flags & tu.RESET)
    ref_out, ref_hist, _ = tu.expected(case)
    src = torch.from_numpy(case.img.copy()).to(ctx.device)
    depth = torch.from_numpy(case.depth.view(np.int32).copy()).to(ctx.device)
    hin = torch.from_numpy(case.hist.view(np.int16).copy()).to(ctx.device)
    out, hout = torch.zeros((case.Ho, case.Wo, 4), dtype=torch.uint8, device=ctx.device), torch.zeros_like(hin)
    pcb = case.pass_constants(lib)
    p = lib.TaaUpscaleParams.default(blend=case.blend, flags=case.flags)
    cur, prev = (C.c_float * 16)(*case.cur), (C.c_float * 16)(*case.prev)

    def call():
        s = torch.cuda.current_stream(ctx.device)
        lib.check(lib.lib.crychic_taa_upscale(ctx.handle, C.byref(pcb), cur, prev, case.jitter[0], case.jitter[1], C.c_void_p(depth.data_ptr()),
                                              C.c_void_p(src.data_ptr()), case.Wi, case.Hi, C.c_void_p(hin.data_ptr()), C.c_void_p(hout.data_ptr()),
                                              C.c_void_p(out.data_ptr()), case.Wo, case.Ho, 0, case.Ho, C.byref(p), C.c_void_p(s.cuda_stream)))
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


def test_convergence_orderings_on_the_device(dev):
    from test_taa_upscale_host import convergence
    acc, bil, neg = convergence(lambda c: tu.run_device(dev, c))
    want = convergence(lambda c: tu.checker(c)[:2])
    print("mean absolute error on the device: %.2f accumulated, %.2f bilinear, %.2f with the jitter negated" % (acc, bil, neg))
    assert acc < bil and acc < neg and (acc, bil, neg) == want
