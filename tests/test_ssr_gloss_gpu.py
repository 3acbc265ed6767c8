"""crychic_ssr_pyramid and crychic_ssr_glossy on the device: the kernels against the checker (tests/ssr_gloss_ref) byte for byte on the
pyramid's sizes and on the corpus of the CPU tier under the three gloss settings, behind guard bytes, on misaligned planes, in every
format mix and in row ranges; the definition's known answers and its level anchor on the device's output; the refusals with a
context; and the passes behind Crychic.Draw -- ssr + ssrGloss alone and in front of the fog, the calls by name, ssrGloss without ssr,
the switch unset again, and replayed from a graph."""
import ctypes as C

import numpy as np
import pytest

import fog_lib as fg
import ssr_gloss_lib as gl
import ssr_lib as sl
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture
from recorder_lib import Recorder

pytestmark = pytest.mark.gpu


def device_pyramid(dev, planes, src, W, H, levels):
    """crychic_ssr_pyramid of the device frame `src` into a guarded workspace of GUARD: the workspace's view (not yet synchronised)."""
    lib, ctx, torch = dev
    need = int(lib.lib.crychic_ssr_pyramid_bytes(W, H, levels))
    ws = planes.blank("pyramid", (max(need, 16),))
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_ssr_pyramid(ctx.handle, C.c_void_p(src.data_ptr()), W, H, levels, C.c_void_p(ws.data_ptr()), need, C.c_void_p(s.cuda_stream)))
    return ws


def run_pyramid(dev, img, levels, misalign=0):
    """The device's pyramid of `img`, the frame `misalign` bytes past a 256-byte boundary: a flat uint8 array as gl.pyramid gives it,
    the guards and the frame checked."""
    lib, ctx, torch = dev
    H, W = img.shape[:2]
    planes = DevicePlanes(dev)
    ws = device_pyramid(dev, planes, planes.upload("input", img, misalign), W, H, levels)
    torch.cuda.current_stream(ctx.device).synchronize()
    planes.verify()
    return ws.cpu().numpy()


def run_device(dev, frame, img, params=None, gloss=None, row0=0, rows=None, mix=0, misalign=0):
    """crychic_ssr_pyramid then crychic_ssr_glossy on guarded device copies of `img`, the depth plane and the G-buffer planes in the
    formats of `mix`, the frame and depth planes `misalign` bytes past a 256-byte boundary (the G-buffer planes: one texel, if any);
    returns (the output plane, the pyramid) as numpy, the guards and the inputs checked."""
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
    q = None if gloss is None else lib.SsrGlossParams.default(**gloss)
    levels = int(gl.gloss_array(gloss)[1])
    ws = device_pyramid(dev, planes, src, W, H, levels)
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_ssr_glossy(ctx.handle, C.byref(pcb), C.c_void_p(g[0].data_ptr()), C.c_void_p(g[1].data_ptr()), C.c_void_p(g[2].data_ptr()),
                                         C.c_void_p(depth.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                         C.c_void_p(out.data_ptr()), W, H, row0, H - row0 if rows is None else rows, sl.format_flags(mix),
                                         None if p is None else C.byref(p), None if q is None else C.byref(q), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return out.cpu().numpy().reshape(img.shape), ws.cpu().numpy()


# ---- the pyramid alone --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", gl.PYRAMID_SIZES, ids=lambda s: "%dx%d" % s)
def test_pyramid_device_equals_checker(dev, size):
    W, H = size
    img = gl.pyramid_frame(W, H)
    for levels, misalign in ((8, 0), (8, 4), (8, 12), (3, 0), (1, 4)):
        assert np.array_equal(run_pyramid(dev, img, levels, misalign), gl.pyramid(img, levels)), (size, levels, misalign)


def test_pyramid_known_answers(dev):
    gl.check_pyramid_answers(lambda img, levels: gl.level_views(run_pyramid(dev, img, levels), img.shape[1], img.shape[0], levels))


# ---- the pass -----------------------------------------------------------------------------------------------------------------------

def small(img):
    """None above 128 x 96 but the thin frames."""
    H, W = img.shape[:2]
    return W * H <= 128 * 96 or min(W, H) <= 3


@pytest.mark.parametrize("gname", list(gl.GLOSS_SETS))
def test_device_equals_checker(dev, gname):
    """Every small case of the corpus under one misalignment, chosen so that the three settings between them take all three."""
    gi = list(gl.GLOSS_SETS).index(gname)
    ran = 0
    for ci, (name, frame, img, pn, mix) in enumerate(sl.corpus()):
        if not small(img):
            continue
        pyr, ref, _, _ = gl.expected(name, gname)
        misalign = (0, 4, 12)[(ci + gi) % 3]
        got, ws = run_device(dev, frame, img, sl.PARAM_SETS[pn], None if gname == "default" and misalign == 0 else gl.GLOSS_SETS[gname], mix=mix,
                             misalign=misalign)
        assert np.array_equal(ws, pyr), "%s under %s: the pyramid differs" % (name, gname)
        assert np.array_equal(got, ref), "%s under %s, planes %d bytes past a 256-byte boundary: %d bytes differ" % (
            name, gname, misalign, int((got != ref).sum()))
        ran += 1
    assert ran >= 50


def test_known_answers(dev):
    from test_ssr_gloss_host import glossy_answers
    glossy_answers(lambda f, i, p, g: run_device(dev, f, i, p, g)[0])


@pytest.mark.parametrize("size", [(128, 96), (70, 38)])
def test_level_anchor(dev, size):
    W, H = size
    frame, img, truth = gl.anchor_scene(W, H)
    out, _, dbg = gl.checker(frame, img, sl.PARAM_SETS["mirror_n64"], gl.ANCHOR_GLOSS)
    gl.check_level_anchor(W, H, dbg, truth)
    got, _ = run_device(dev, frame, img, sl.PARAM_SETS["mirror_n64"], gl.ANCHOR_GLOSS)
    assert np.array_equal(got, out), "the device's frame is not the one whose levels were checked"


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 96), (0, 7, 12, 95, 96)])
def test_row_ranges_stitch_to_the_whole_frame(dev, split):
    by_name = {c[0]: c for c in sl.corpus()}
    for name, gname, misalign in (("scene128_mirror_n64", "c16_l8", 0), ("scene128_long_n63", "c05_l3", 4)):
        _, frame, img, pn, _ = by_name[name]
        _, whole, _, _ = gl.expected(name, gname)
        stitched = np.full(img.shape, sl.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got, _ = run_device(dev, frame, img, sl.PARAM_SETS[pn], gl.GLOSS_SETS[gname], row0=row0, rows=end - row0, misalign=misalign)
            assert (got[:row0] == sl.GUARD).all() and (got[end:] == sl.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
        assert np.array_equal(stitched, whole), name
    got, _ = run_device(dev, frame, img, sl.PARAM_SETS[pn], gl.GLOSS_SETS[gname], row0=96, rows=0)
    assert (got == sl.GUARD).all()


def test_format_mixes_match_the_widened_planes(dev):
    by_name = {c[0]: c for c in sl.corpus()}
    _, ref, n, _ = gl.expected("130x9_formats_0", "c16_l8")
    assert n["lq_positive"] > 0
    for mix in range(8):
        _, frame, img, pn, m = by_name["130x9_formats_%d" % mix]
        assert m == mix and np.array_equal(run_device(dev, frame, img, sl.PARAM_SETS[pn], gl.GLOSS_SETS["c16_l8"], mix=mix)[0], ref), mix


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    a = torch.zeros((32, 64, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((32, 65, 4), sl.GUARD, dtype=torch.uint8, device=ctx.device)
    need = int(lib.lib.crychic_ssr_pyramid_bytes(64, 32, 6))
    w = torch.full((need + 64,), sl.GUARD, dtype=torch.uint8, device=ctx.device)
    d = torch.zeros((32, 64), dtype=torch.int32, device=ctx.device)
    g = torch.zeros((3, 32, 64, 4), dtype=torch.float32, device=ctx.device)
    pa, pb, pd, pw = (C.c_void_p(t.data_ptr()) for t in (a, b, d, w))
    g0, g1, g2 = (C.c_void_p(g[k].data_ptr()) for k in range(3))
    cb = sl.camera_constants(64, 32)
    f, py = lib.lib.crychic_ssr_glossy, lib.lib.crychic_ssr_pyramid

    def msg():
        return lib.lib.crychic_last_error().decode()
    assert py(ctx.handle, None, 64, 32, 6, pw, need, None) == -1
    assert py(ctx.handle, pa, 64, 32, 6, None, need, None) == -1
    assert py(ctx.handle, pa, 64, 32, 6, C.c_void_p(w.data_ptr() + 8), need, None) == -1 and "aligned" in msg()
    assert py(ctx.handle, pa, 64, 32, 6, pw, need - 1, None) == -1 and "needs" in msg()
    assert py(ctx.handle, pa, 64, 32, 9, pw, need, None) == -1 and "levels" in msg()
    assert py(ctx.handle, pa, 64, 32, 6, pa, need, None) == -1 and "overlaps" in msg()
    assert py(ctx.handle, pa, 0, 32, 6, pw, need, None) == -1
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pw, need, pa, 64, 32, 0, 32, 0, None, None, None) == -1 and "overlap" in msg()
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, None, need, pb, 64, 32, 0, 32, 0, None, None, None) == -1
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pw, need - 1, pb, 64, 32, 0, 32, 0, None, None, None) == -1 and "needs" in msg()
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pb, need, pb, 64, 32, 0, 32, 0, None, None, None) == -1 and "overlaps" in msg()
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pw, need, pb, 64, 32, 1, 32, 0, None, None, None) == -1
    bad = lib.SsrGlossParams.default(coneScale=17.0)
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pw, need, pb, 64, 32, 0, 32, 0, None, C.byref(bad), None) == -1 and "coneScale" in msg()
    bad = lib.SsrGlossParams.default(levels=7)
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pw, need, pb, 64, 32, 0, 32, 0, None, C.byref(bad), None) == -1 and "needs" in msg()
    bad = lib.SsrParams.default(steps=65)
    assert f(ctx.handle, C.byref(cb), g0, g1, g2, pd, pa, pw, need, pb, 64, 32, 0, 32, 0, C.byref(bad), None, None) == -1 and "steps" in msg()
    torch.cuda.synchronize()
    assert bool((b == sl.GUARD).all()) and bool((w == sl.GUARD).all()), "a refused call wrote"


# ---- behind Crychic.Draw -----------------------------------------------------------------------------------------------------------

LIGHTING = ["crychic_draw_hot_path_point_shadows"]
GLOSSY = ["crychic_ssr_pyramid_bytes", "crychic_ssr_pyramid", "crychic_ssr_glossy"]
MINE = dict(coneScale=1.0, levels=5)


@pytest.fixture(scope="module")
def app_frame(dev):
    """Two Crychic over the planes of the 128 x 96 synthetic scene with its roughness scaled by a quarter -- `app` for Draw(), `hand`
    whose switches are never set --, the frame Draw() gives without the passes, and what the passes read of the scene."""
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
    assert app.ssrGloss is None and app.mSsrPyramid is None
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.cpu().numpy().copy()
    depth = planes["depth"].cpu().numpy().view(np.uint32)
    frame = sl.Frame.from_pass_cb(app.mMainPassCB, *(planes["g%d" % k].cpu().numpy() for k in range(3)), depth)
    fog_frame = fg.Frame.from_pass_cb(app.mMainPassCB, depth, planes["shadow"].cpu().numpy().view(np.uint32))
    return app, hand, plain, frame, fog_frame


def test_draw_with_ssr_gloss(dev, app_frame):
    lib, ctx, torch = dev
    from crychic_renderer_amd import SsrGlossParams, SsrParams
    app, hand, plain, frame, fog_frame = app_frame
    sharp, n, _ = sl.checker(frame, plain)
    want, n, _ = gl.checker(frame, plain, None, MINE)
    assert n["lq_positive"] > 0 and not np.array_equal(want, sharp), "the cone changes nothing on the scene"
    app.ssr, app.ssrGloss = True, SsrGlossParams.default(**MINE)
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferSSR.cpu().numpy(), want), "mBackBufferSSR is not the checker's frame over the Draw() without the pass"
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain) and app.final_frame() is app.mBackBufferSSR
        # against the passes issued by hand on a second object
        hand.Draw()
        assert hand.ssr_pyramid(levels=MINE["levels"]) is hand.mSsrPyramid
        assert hand.screen_space_reflections(gloss=SsrGlossParams.default(**MINE)) is hand.mBackBufferSSR
        torch.cuda.synchronize()
        assert torch.equal(app.mBackBufferSSR, hand.mBackBufferSSR) and torch.equal(app.mSsrPyramid, hand.mSsrPyramid)
        n_bytes = int(lib.lib.crychic_ssr_pyramid_bytes(128, 96, MINE["levels"]))
        assert np.array_equal(app.mSsrPyramid.cpu().numpy()[:n_bytes], gl.pyramid(plain, MINE["levels"])[:n_bytes])
        # True: the defaults, the sharp pass; the SsrParams still reach the pass
        app.ssrGloss = True
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferSSR.cpu().numpy(), gl.checker(frame, plain)[0])
        mine = dict(maxDistance=12.0, thickness=1.5, maxRoughness=1.0, steps=48, edgeFade=8, intensity=200)
        app.ssr, app.ssrGloss = SsrParams.default(**mine), SsrGlossParams.default(**MINE)
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferSSR.cpu().numpy(), gl.checker(frame, plain, dict(sl.DEFAULTS, **mine), MINE)[0])
        # in front of the fog
        app.ssr, app.fog = True, True
        app.Draw()
        hand.Draw()
        hand.ssr_pyramid(levels=MINE["levels"])
        f = hand.screen_space_reflections(gloss=SsrGlossParams.default(**MINE))
        assert hand.apply_fog(src=f) is f
        torch.cuda.synchronize()
        fogged, _ = fg.checker(fog_frame, want)
        assert not np.array_equal(fogged, want) and np.array_equal(app.mBackBufferSSR.cpu().numpy(), fogged)
        assert torch.equal(app.mBackBufferSSR, hand.mBackBufferSSR) and np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
    finally:
        app.ssr, app.ssrGloss, app.fog = None, None, None
    assert app.final_frame() is app.mBackBuffer and not app._post and not hand._post
    # the method on its own: gloss=None is crychic_ssr
    out = torch.full_like(app.mBackBuffer, sl.GUARD)
    assert app.screen_space_reflections(out=out, row0=7, rows=50, gloss=None) is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[7:57], sharp[7:57]) and (got[:7] == sl.GUARD).all() and (got[57:] == sl.GUARD).all()


def test_calls_by_name_and_the_switch_unset_again(dev, app_frame, monkeypatch):
    lib, ctx, torch = dev
    from crychic_renderer_amd import SsrGlossParams, renderer
    app, hand, plain, frame, _ = app_frame
    rec = Recorder(renderer.lib)
    monkeypatch.setattr(renderer, "lib", rec)
    try:
        app.ssrGloss = SsrGlossParams.default(**MINE)           # without ssr: refused with nothing issued
        with pytest.raises(lib.CrychicError, match="ssrGloss is set and ssr is not"):
            app.Draw()
        assert rec.calls == []
        app.ssr = True
        app.Draw()
        assert rec.calls == LIGHTING + GLOSSY, rec.calls
        app.fog = True
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + GLOSSY + ["crychic_fog"], rec.calls
        with pytest.raises(lib.CrychicError, match="fog is set"):
            app.Draw(row0=0, rows=48)
        app.fog = None
        with pytest.raises(lib.CrychicError, match="ssr is set"):
            app.Draw(row0=0, rows=48)
        app.ssrGloss = None                                     # unset again: the earlier calls and bytes
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING + ["crychic_ssr"], rec.calls
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferSSR.cpu().numpy(), sl.checker(frame, plain)[0])
        app.ssr = None
        del rec.calls[:]
        app.Draw()
        assert rec.calls == LIGHTING and not app._post, rec.calls
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "with the switches unset Draw() gives the frame it gave before"
    finally:
        app.ssr, app.ssrGloss, app.fog = None, None, None


def test_draw_replays_from_a_graph(dev, app_frame):
    lib, ctx, torch = dev
    from crychic_renderer_amd import SsrGlossParams
    app, hand, plain, frame, _ = app_frame
    want, _, _ = gl.checker(frame, plain, None, MINE)
    app.ssr, app.ssrGloss = True, SsrGlossParams.default(**MINE)
    try:
        app.Draw()                          # before the capture: the code objects loaded, the buffers allocated
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            app.Draw()
        for _ in range(2):
            app.mBackBuffer.zero_()
            app.mBackBufferSSR.zero_()
            app.mSsrPyramid.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(app.mBackBufferSSR.cpu().numpy(), want)
    finally:
        app.ssr, app.ssrGloss = None, None
