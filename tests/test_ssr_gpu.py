"""crychic_ssr on the device: the kernel against the checker (tests/ssr_ref) byte for byte on the corpus of the CPU tier, behind guard
bytes, on misaligned planes, in every format mix and in row ranges; the definition's known answers and its mirror anchor on the
device's output; the refusals with a context; and the pass behind Crychic.Draw -- alone, in front of the fog, in front of all six
other switches, with the switch unset again, and replayed from a graph."""
import ctypes as C

import numpy as np
import pytest

import fog_lib as fg
import ssr_lib as sl
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture
from recorder_lib import Recorder

pytestmark = pytest.mark.gpu


def run_device(dev, frame, img, params=None, row0=0, rows=None, mix=0, misalign=0):
    """crychic_ssr on guarded device copies of `img`, the depth plane and the G-buffer planes in the formats of `mix`, the frame and
    depth planes `misalign` bytes past a 256-byte boundary (the G-buffer planes: one texel, if any); returns the output plane as
    numpy, the guards and the inputs checked."""
    lib, ctx, torch = dev
    H, W = img.shape[:2]
    planes = DevicePlanes(dev)
    src = planes.upload("input", img, misalign)
    depth = planes.upload("depth", frame.depth, misalign)
    g = []
    for k in range(3):
        p = frame.plane(k, mix)
        g.append(planes.upload("g%d" % k, p, p.dtype.itemsize * 4 if misalign else 0))
    out = planes.blank("out", img.shape, np.uint8, misalign)
    pcb = frame.pass_constants(lib)
    p = None if params is None else lib.SsrParams.default(**dict(sl.DEFAULTS, **params))
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_ssr(ctx.handle, C.byref(pcb), C.c_void_p(g[0].data_ptr()), C.c_void_p(g[1].data_ptr()), C.c_void_p(g[2].data_ptr()),
                                  C.c_void_p(depth.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), W, H, row0,
                                  H - row0 if rows is None else rows, sl.format_flags(mix), None if p is None else C.byref(p),
                                  C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return out.cpu().numpy().reshape(img.shape)


@pytest.mark.parametrize("pname", list(sl.PARAM_SETS))
def test_device_equals_checker(dev, pname):
    for name, frame, img, pn, mix in sl.corpus():
        if pn != pname:
            continue
        ref, _, _ = sl.expected(name)
        for misalign in (0, 4, 12):
            got = run_device(dev, frame, img, None if pn == "default" and misalign == 0 else sl.PARAM_SETS[pn], mix=mix, misalign=misalign)
            assert np.array_equal(got, ref), "%s, planes %d bytes past a 256-byte boundary: %d bytes differ" % (name, misalign, int((got != ref).sum()))


def test_known_answers(dev):
    from test_ssr_host import answers
    answers(lambda f, i, p: run_device(dev, f, i, p))


@pytest.mark.parametrize("size", [(128, 96), (70, 38)])
def test_mirror_anchor(dev, size):
    W, H = size
    frame, img, truth = sl.mirror_scene(W, H)
    _, _, dbg = sl.checker(frame, img, sl.PARAM_SETS["mirror_n64"])
    sl.check_mirror(W, H, run_device(dev, frame, img, sl.PARAM_SETS["mirror_n64"]), dbg, frame, img, truth)


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 190)])
def test_row_ranges_stitch_to_the_whole_frame(dev, split):
    by_name = {c[0]: c for c in sl.corpus()}
    for name, misalign in (("322x190_ramp_long_n63", 0), ("322x190_zeros_mirror_n64", 4)):
        _, frame, img, pn, _ = by_name[name]
        whole, _, _ = sl.expected(name)
        stitched = np.full(img.shape, sl.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got = run_device(dev, frame, img, sl.PARAM_SETS[pn], row0=row0, rows=end - row0, misalign=misalign)
            assert (got[:row0] == sl.GUARD).all() and (got[end:] == sl.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
        assert np.array_equal(stitched, whole), name
    _, frame, img, pn, _ = by_name["scene128_default"]
    whole, _, _ = sl.expected("scene128_default")
    for row0, rows in ((0, 1), (5, 1), (6, 83), (96, 0)):
        got = run_device(dev, frame, img, sl.PARAM_SETS[pn], row0=row0, rows=rows)
        assert np.array_equal(got[row0:row0 + rows], whole[row0:row0 + rows])
        assert (got[:row0] == sl.GUARD).all() and (got[row0 + rows:] == sl.GUARD).all()


def test_format_mixes_match_the_widened_planes(dev):
    by_name = {c[0]: c for c in sl.corpus()}
    ref, n, _ = sl.expected("130x9_formats_0")
    assert n["hit_first"] + n["hit_later"] > 0
    for mix in range(8):
        _, frame, img, pn, m = by_name["130x9_formats_%d" % mix]
        assert m == mix and np.array_equal(run_device(dev, frame, img, sl.PARAM_SETS[pn], mix=mix), ref), mix


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    a = torch.zeros((32, 64, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((32, 65, 4), sl.GUARD, dtype=torch.uint8, device=ctx.device)
    d = torch.zeros((32, 64), dtype=torch.int32, device=ctx.device)
    g = torch.zeros((3, 32, 64, 4), dtype=torch.float32, device=ctx.device)
    pa, pb, pd = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(d.data_ptr())
    g0, g1, g2 = (C.c_void_p(g[k].data_ptr()) for k in range(3))
    cb = sl.camera_constants(64, 32)
    f = lib.lib.crychic_ssr

    def msg():
        return lib.lib.crychic_last_error().decode()
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pa, 64, 32, 0, 32, 0, None, None) == -1 and "overlap" in msg()
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, C.c_void_p(a.data_ptr() + 4), 64, 32, 0, 32, 0, None, None) == -1 and "overlap" in msg()
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, None, pb, 64, 32, 0, 32, 0, None, None) == -1
    assert f(ctx.handle, C.byref(cb), g0, None, g2, pd, pa, pb, 64, 32, 0, 32, 0, None, None) == -1
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pb, 64, 32, 1, 32, 0, None, None) == -1
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pb, 64, 32, 0, 32, 0x100, None, None) == -1 and "flags" in msg()
    bad = lib.SsrParams.default(steps=65)
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pb, 64, 32, 0, 32, 0, C.byref(bad), None) == -1 and "steps" in msg()
    cb.Proj[11] = 0.0
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pb, 64, 32, 0, 32, 0, None, None) == -1 and "Proj[11]" in msg()
    torch.cuda.synchronize()
    assert bool((b == sl.GUARD).all()), "a refused call wrote"


# ---- behind Crychic.Draw -----------------------------------------------------------------------------------------------------------

OTHERS = ("fog", "temporalAA", "depthOfField", "motionBlur", "bloom", "antiAliasing")          # in the chain's order
BUFFER = dict(temporalAA="mBackBufferTAA", depthOfField="mBackBufferDoF", motionBlur="mBackBufferMB", bloom="mBackBufferBloom",
              antiAliasing="mBackBufferAA")
LIGHTING = ["crychic_draw_hot_path_point_shadows"]


@pytest.fixture(scope="module")
def app_frame(dev):
    """Two Crychic over the planes of the 128 x 96 synthetic scene with its roughness scaled by a quarter -- `app` for Draw(), `hand`
    whose switches are never set --, the frame Draw() gives without the pass, and what the passes read of the scene."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    W, H, SD = 128, 96, 256
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    planes["g1"][..., 3] *= 0.25
    apps = []
    for _ in range(2):
        a = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
        a.load_scene(planes)
        a.blurCount, a.numDirLights, a.flags = 3, 3, LIGHT_SKY
        apps.append(a)
    app, hand = apps
    assert app.ssr is None and app.mBackBufferSSR is None
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.cpu().numpy().copy()
    depth = planes["depth"].cpu().numpy().view(np.uint32)
    frame = sl.Frame.from_pass_cb(app.mMainPassCB, *(planes["g%d" % k].cpu().numpy() for k in range(3)), depth)
    fog_frame = fg.Frame.from_pass_cb(app.mMainPassCB, depth, planes["shadow"].cpu().numpy().view(np.uint32))
    return app, hand, plain, frame, fog_frame


def test_draw_with_ssr(dev, app_frame):
    lib, ctx, torch = dev
    from crychic_renderer_amd import SsrParams
    app, hand, plain, frame, _ = app_frame
    want, n, _ = sl.checker(frame, plain)
    assert n["hit_first"] + n["hit_later"] > 0 and not np.array_equal(want, plain), "the scene reflects nothing"
    app.ssr = True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferSSR.cpu().numpy(), want), "mBackBufferSSR is not the checker's frame over the Draw() without the pass"
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain) and app.final_frame() is app.mBackBufferSSR
        # an SsrParams: its values reach the pass
        mine = dict(maxDistance=12.0, thickness=1.5, maxRoughness=1.0, steps=48, edgeFade=8, intensity=200)
        app.ssr = SsrParams.default(**mine)
        app.Draw()
        torch.cuda.synchronize()
        want_mine, _, _ = sl.checker(frame, plain, dict(sl.DEFAULTS, **mine))
        assert not np.array_equal(want_mine, want) and np.array_equal(app.mBackBufferSSR.cpu().numpy(), want_mine)
    finally:
        app.ssr = None
    assert app.final_frame() is app.mBackBuffer
    # the method on its own: another destination and a row range; mBackBuffer stays
    out = torch.full_like(app.mBackBuffer, sl.GUARD)
    assert app.screen_space_reflections(out=out, row0=7, rows=50) is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[7:57], want[7:57]) and (got[:7] == sl.GUARD).all() and (got[57:] == sl.GUARD).all()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
    with pytest.raises(lib.CrychicError):
        app.screen_space_reflections(src=app.mBackBuffer, out=app.mBackBuffer)      # in place is refused


def test_ssr_then_fog(dev, app_frame):
    lib, ctx, torch = dev
    app, hand, plain, frame, fog_frame = app_frame
    reflected, _, _ = sl.checker(frame, plain)
    want, n = fg.checker(fog_frame, reflected)
    assert not np.array_equal(want, reflected)
    app.ssr, app.fog = True, True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferSSR.cpu().numpy(), want), "mBackBufferSSR is not the fog checker's frame over the SSR checker's"
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "mBackBuffer is no longer the plain frame"
        assert app.final_frame() is app.mBackBufferSSR
    finally:
        app.ssr, app.fog = None, None


def test_ssr_with_all_six_other_switches(dev, app_frame):
    """Against the same passes issued by hand on a second object, over two frames (the temporal pass's first is a RESET frame)."""
    lib, ctx, torch = dev
    import bloom_lib
    import motion_blur_lib as mbl
    app, hand, plain, frame, _ = app_frame
    W, H = 128, 96
    bloom = lib.BloomParams.default(**bloom_lib.SCENE_PARAMS)
    cur = np.array(app.mMainPassCB.ViewProj[:], np.float32)
    moved = mbl.camera_matrices(W, H, cam=mbl.moved_camera(W, H, dx=-0.3, yaw=0.02))[0]
    for a in (app, hand):
        a.set_frame_view_proj(moved)
        a.set_frame_view_proj(cur)
    app.ssr = True
    for s in OTHERS:
        setattr(app, s, bloom if s == "bloom" else True)
    try:
        for k in range(2):
            app.Draw()
            hand.Draw()
            f = hand.screen_space_reflections()
            assert f is hand.mBackBufferSSR and hand.apply_fog(src=f) is f
            f = hand.temporal_aa(cur, moved, src=f, reset=k == 0)
            f = hand.depth_of_field(src=f)
            f = hand.motion_blur(cur, moved, src=f)
            f = hand.apply_bloom(src=f, params=bloom)
            f = hand.antialias(src=f)
            torch.cuda.synchronize()
            assert torch.equal(app.mBackBuffer, hand.mBackBuffer) and np.array_equal(app.mBackBuffer.cpu().numpy(), plain), k
            assert torch.equal(app.mBackBufferSSR, hand.mBackBufferSSR) and not torch.equal(app.mBackBufferSSR, app.mBackBuffer), k
            for s in OTHERS[1:]:
                assert torch.equal(getattr(app, BUFFER[s]), getattr(hand, BUFFER[s])), (k, s)
            assert app.final_frame() is app.mBackBufferAA and f is hand.mBackBufferAA
        assert not hand._post
    finally:
        app.ssr = None
        for s in OTHERS:
            setattr(app, s, None)


def test_unset_again_draw_is_the_plain_frame_and_the_same_calls(dev, app_frame, monkeypatch):
    lib, ctx, torch = dev
    from crychic_renderer_amd import renderer
    app, hand, plain, frame, _ = app_frame
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        app.ssr = True
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_ssr"], rec.calls
        app.fog = True
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_ssr", "crychic_fog"], rec.calls
        app.ssr = None
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_fog"], rec.calls
        app.fog = None
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING and not app._post, rec.calls
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "with the switch unset Draw() gives the frame it gave before"
        del rec.calls[:]
        app.Draw(row0=0, rows=48)               # without it a strip is a strip
        assert rec.calls == LIGHTING
        torch.cuda.synchronize()
    finally:
        app.ssr, app.fog = None, None


def test_strip_or_shared_draw_raises(dev, app_frame, monkeypatch):
    lib, ctx, torch = dev
    from crychic_renderer_amd import renderer
    app, hand, plain, frame, _ = app_frame
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    app.ssr = True
    try:
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError, match="ssr is set"):
                app.Draw(**kw)
        assert rec.calls == []
        app.fog = True                          # an earlier switch's message does not change
        with pytest.raises(lib.CrychicError, match="fog is set"):
            app.Draw(row0=0, rows=48)
        app.fog = None
        app.Draw(row0=0, rows=96)               # the whole frame, spelled out
        assert rec.calls == LIGHTING + ["crychic_ssr"]
        torch.cuda.synchronize()
    finally:
        app.ssr, app.fog = None, None


def test_draw_and_pass_replay_from_a_graph(dev, app_frame):
    lib, ctx, torch = dev
    app, hand, plain, frame, _ = app_frame
    want, _, _ = sl.checker(frame, plain)
    app.ssr = True
    try:
        app.Draw()                          # before the capture: the code objects loaded, mBackBufferSSR allocated
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            app.Draw()
        for _ in range(2):
            app.mBackBuffer.zero_()
            app.mBackBufferSSR.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(app.mBackBufferSSR.cpu().numpy(), want)
    finally:
        app.ssr = None
