"""crychic_fog on the device: the kernel against the checker (tests/fog_ref) byte for byte on the corpus of the CPU tier, behind guard
bytes, in place and out of place, on misaligned planes and in row ranges; and the pass behind Crychic.Draw -- alone, in front of the
anti-aliasing, and replayed from a graph."""
import ctypes as C

import numpy as np
import pytest

import fog_lib as fg
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu

_MAPS = {}


def device_maps(dev, frame):
    """The frame's four maps on the device, uploaded once per map array."""
    lib, ctx, torch = dev
    key = id(frame.maps)
    if key not in _MAPS:
        _MAPS[key] = (frame.maps, torch.from_numpy(frame.maps.view(np.int32).copy()).to(ctx.device))
    t = _MAPS[key][1]
    return t, (C.c_void_p * 4)(*[t[j].data_ptr() for j in range(4)])


def run_device(dev, frame, img, params=None, row0=0, rows=None, in_place=False, misalign=0):
    """crychic_fog on guarded device copies of `img` and the depth plane; returns the output plane as numpy, the guards and the inputs
    checked."""
    lib, ctx, torch = dev
    H, W = img.shape[:2]
    planes = DevicePlanes(dev)
    src = planes.upload("input", img, misalign, writable=in_place)
    depth = planes.upload("depth", frame.depth, misalign)
    out = src if in_place else planes.blank("out", img.shape, np.uint8, misalign)
    maps, mp = device_maps(dev, frame)
    pcb = frame.pass_constants(lib)
    p = None
    if params is not None:
        q = dict(fg.DEFAULTS, **params)
        p = lib.FogParams.default(**q)
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_fog(ctx.handle, C.byref(pcb), C.c_void_p(depth.data_ptr()), mp, frame.dim, C.c_void_p(src.data_ptr()),
                                  C.c_void_p(out.data_ptr()), W, H, row0, H - row0 if rows is None else rows, None if p is None else C.byref(p),
                                  C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    assert np.array_equal(maps.cpu().numpy().view(np.uint32), frame.maps), "a map changed"
    return out.cpu().numpy().reshape(img.shape)


@pytest.mark.parametrize("pname", list(fg.PARAM_SETS))
def test_device_equals_checker(dev, pname):
    for name, frame, img, pn, _ in fg.corpus():
        if pn != pname:
            continue
        ref, _ = fg.expected(name)
        got = run_device(dev, frame, img, None if pn == "default" else fg.PARAM_SETS[pn])
        assert np.array_equal(got, ref), "%s: %d bytes differ" % (name, int((got != ref).sum()))
        got = run_device(dev, frame, img, fg.PARAM_SETS[pn], in_place=True, misalign=4)
        assert np.array_equal(got, ref), "%s in place, planes 4 bytes past a 16-byte boundary: %d bytes differ" % (name, int((got != ref).sum()))


def test_misaligned_planes_out_of_place(dev):
    by_name = {c[0]: c for c in fg.corpus()}
    for name in ("scene128_default", "golden64_bright_n63", "322x190_map100_zeros_random_far_n2"):
        _, frame, img, pn, _ = by_name[name]
        ref, _ = fg.expected(name)
        assert np.array_equal(run_device(dev, frame, img, fg.PARAM_SETS[pn], misalign=12), ref), name


def test_known_answers(dev):
    from test_fog_host import answers
    answers(lambda f, i, p: run_device(dev, f, i, p))
    answers(lambda f, i, p: run_device(dev, f, i, p, in_place=True))


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 190)])
def test_row_ranges_stitch_to_the_whole_frame(dev, split):
    by_name = {c[0]: c for c in fg.corpus()}
    for name, misalign in (("322x190_map100_zeros_random_far_n2", 0), ("322x190_map100_random_step_thin_n1", 4)):
        _, frame, img, pn, _ = by_name[name]
        whole, _ = fg.expected(name)
        stitched = np.full(img.shape, fg.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got = run_device(dev, frame, img, fg.PARAM_SETS[pn], row0=row0, rows=end - row0, misalign=misalign)
            assert (got[:row0] == fg.GUARD).all() and (got[end:] == fg.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
        assert np.array_equal(stitched, whole), name
    _, frame, img, pn, _ = by_name["scene128_default"]
    whole, _ = fg.expected("scene128_default")
    for row0, rows in ((0, 1), (5, 1), (6, 83), (96, 0)):              # in place: the other rows keep the input
        got = run_device(dev, frame, img, fg.PARAM_SETS[pn], row0=row0, rows=rows, in_place=True)
        assert np.array_equal(got[row0:row0 + rows], whole[row0:row0 + rows])
        assert np.array_equal(got[:row0], img[:row0]) and np.array_equal(got[row0 + rows:], img[row0 + rows:])


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    a = torch.zeros((32, 64, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((32, 65, 4), fg.GUARD, dtype=torch.uint8, device=ctx.device)
    d = torch.zeros((32, 64), dtype=torch.int32, device=ctx.device)
    m = torch.zeros((4, 8, 8), dtype=torch.int32, device=ctx.device)
    mp = (C.c_void_p * 4)(*[m[j].data_ptr() for j in range(4)])
    pa, pb, pd = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(d.data_ptr())
    cb = fg.camera_constants(64, 32, 8)
    f = lib.lib.crychic_fog
    assert f(ctx.handle, C.byref(cb), pd, mp, 8, pa, C.c_void_p(a.data_ptr() + 4), 64, 32, 0, 32, None, None) == -1
    assert "overlap" in lib.lib.crychic_last_error().decode()
    assert f(ctx.handle, C.byref(cb), pd, mp, 8, None, pb, 64, 32, 0, 32, None, None) == -1
    assert f(ctx.handle, C.byref(cb), pd, mp, 0, pa, pb, 64, 32, 0, 32, None, None) == -1
    assert f(ctx.handle, C.byref(cb), pd, mp, 8, pa, pb, 64, 32, 1, 32, None, None) == -1
    bad = lib.FogParams.default(steps=65)
    assert f(ctx.handle, C.byref(cb), pd, mp, 8, pa, pb, 64, 32, 0, 32, C.byref(bad), None) == -1 and "steps" in lib.lib.crychic_last_error().decode()
    cb.ShadowTransforms[1][12] = 0.25
    assert f(ctx.handle, C.byref(cb), pd, mp, 8, pa, pb, 64, 32, 0, 32, None, None) == -1 and "affine" in lib.lib.crychic_last_error().decode()
    torch.cuda.synchronize()
    assert bool((b == fg.GUARD).all()), "a refused call wrote"


@pytest.fixture(scope="module")
def app_frame(dev):
    """A Crychic over the 128 x 96 synthetic scene, the frame Draw() gives without the pass, and what the pass reads of the scene."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    W, H, SD = 128, 96, 256
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 3, 3, LIGHT_SKY
    assert app.fog is None
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.cpu().numpy().copy()
    frame = fg.Frame.from_pass_cb(app.mMainPassCB, planes["depth"].cpu().numpy().view(np.uint32), planes["shadow"].cpu().numpy().view(np.uint32))
    return app, plain, frame


def test_draw_with_fog(dev, app_frame):
    lib, ctx, torch = dev
    from crychic_renderer_amd import FogParams
    app, plain, frame = app_frame
    want, n = fg.checker(frame, plain)
    assert n["lit"] > 0 and n["shadowed"] > 0 and not np.array_equal(want, plain), "the scene has no shaft"
    app.fog = True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), want), "mBackBuffer is not the checker's frame over the Draw() without fog"
        # a FogParams: its values reach the pass
        app.fog = FogParams.default(density=0.08, steps=7, sun=(250, 200, 90))
        app.Draw()
        torch.cuda.synchronize()
        want7, _ = fg.checker(frame, plain, dict(fg.DEFAULTS, density=float(np.float32(0.08)), steps=7, sun=(250, 200, 90)))
        assert not np.array_equal(want7, want) and np.array_equal(app.mBackBuffer.cpu().numpy(), want7)
    finally:
        app.fog = None
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "with fog unset Draw() gives the frame it gave before"
    # apply_fog on its own: another destination and a row range; mBackBuffer stays
    out = torch.full_like(app.mBackBuffer, fg.GUARD)
    assert app.apply_fog(out=out, row0=7, rows=50) is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[7:57], want[7:57]) and (got[:7] == fg.GUARD).all() and (got[57:] == fg.GUARD).all()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
    assert app.apply_fog() is app.mBackBuffer                # the defaults: in place
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), want)


def test_fog_then_anti_aliasing(dev, app_frame):
    lib, ctx, torch = dev
    import post_aa_lib as aa
    app, plain, frame = app_frame
    fogged, _ = fg.checker(frame, plain)
    want, n = aa.checker(fogged)
    assert n["horizontal"] + n["vertical"] > 0
    app.fog, app.antiAliasing = True, True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), fogged)
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), want), "mBackBufferAA is not the anti-aliasing checker over the fogged frame"
        assert app.fog is True and app.antiAliasing is True
    finally:
        app.fog, app.antiAliasing = None, None


def test_strip_or_shared_draw_raises(dev, app_frame):
    lib, ctx, torch = dev
    app, plain, frame = app_frame
    app.fog = True
    try:
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError):
                app.Draw(**kw)
        app.Draw(row0=0, rows=96)           # the whole frame, spelled out
    finally:
        app.fog = None
    app.Draw(row0=0, rows=48)               # without it a strip is a strip
    torch.cuda.synchronize()


def test_draw_and_pass_replay_from_a_graph(dev, app_frame):
    lib, ctx, torch = dev
    app, plain, frame = app_frame
    want, _ = fg.checker(frame, plain)
    app.fog = True
    try:
        app.Draw()                          # before the capture: the code objects loaded
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            app.Draw()
        for _ in range(2):
            app.mBackBuffer.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(app.mBackBuffer.cpu().numpy(), want)
    finally:
        app.fog = None
