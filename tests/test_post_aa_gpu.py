"""crychic_antialias on the device: the kernel against the checker (tests/post_aa_ref) byte for byte on the corpus of the CPU tier,
guard bytes, row ranges, both the 16-byte and the dword path, and the pass behind Crychic.Draw -- eager and replayed from a graph."""
import ctypes as C

import numpy as np
import pytest

import post_aa_lib as aa
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu


def run_device(dev, img, params=None, row0=0, rows=None, misalign=0):
    """crychic_antialias on guarded device copies of `img`; returns the output plane as numpy, the guards and the input checked."""
    lib, ctx, torch = dev
    planes = DevicePlanes(dev)
    src = planes.upload("input", img, misalign)
    out = planes.blank("out", img.shape, np.uint8, misalign)
    H, W = img.shape[:2]
    p = None if params is None else lib.AAParams(*(int(v) for v in aa.params_array(params)))
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_antialias(ctx.handle, C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), W, H, row0, H - row0 if rows is None else rows,
                                        None if p is None else C.byref(p), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return out.cpu().numpy().reshape(img.shape)


@pytest.mark.parametrize("pname", list(aa.PARAM_SETS))
def test_device_equals_checker(dev, oracle, pname):
    for name, img in aa.corpus(oracle):
        ref, _ = aa.expected(name, img, pname)
        got = run_device(dev, img, None if pname == "default" else aa.PARAM_SETS[pname])
        assert np.array_equal(got, ref), "%s / %s: %d bytes differ" % (name, pname, int((got != ref).sum()))


def test_scalar_path_on_a_misaligned_plane(dev, oracle):
    """W = 64, 130 and 322 on planes 4 bytes past a 16-byte boundary (the dword path whatever W is), and W = 65 (never the 16-byte
    path)."""
    images = dict(aa.corpus(oracle))
    for name in ("noise_64x32", "rects_64x32", "slant5_h0_130x70", "noise_322x190", "lines_322x190"):
        ref, _ = aa.expected(name, images[name], "default")
        assert np.array_equal(run_device(dev, images[name], misalign=4), ref), name
        assert np.array_equal(run_device(dev, images[name], misalign=12), ref), name
    for name in ("noise_65x33", "slant1_v1_65x33", "alpha_65x33"):
        ref, _ = aa.expected(name, images[name], "default")
        assert images[name].shape[1] == 65 and np.array_equal(run_device(dev, images[name]), ref), name


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 70), (0, 31, 32, 70), (0, 17, 70)])
def test_row_ranges_stitch_to_the_whole_frame(dev, oracle, split):
    images = dict(aa.corpus(oracle))
    for name, H, misalign in (("noise_130x70", 70, 0), ("slant5_v1_130x70", 70, 0), ("noise_130x70", 70, 4)):
        img = images[name]
        whole, _ = aa.expected(name, img, "default")
        stitched = np.full(img.shape, aa.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got = run_device(dev, img, row0=row0, rows=end - row0, misalign=misalign)
            assert (got[:row0] == aa.GUARD).all() and (got[end:] == aa.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
        assert np.array_equal(stitched, whole), name
    img = images["rects_64x32"]                       # the 16-byte path
    whole, _ = aa.expected("rects_64x32", img, "default")
    for row0, rows in ((0, 1), (1, 1), (5, 20), (31, 1), (32, 0)):
        got = run_device(dev, img, row0=row0, rows=rows)
        assert np.array_equal(got[row0:row0 + rows], whole[row0:row0 + rows]) and (got[:row0] == aa.GUARD).all() and (got[row0 + rows:] == aa.GUARD).all()


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    a = torch.zeros((32, 64, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((32, 64, 4), aa.GUARD, dtype=torch.uint8, device=ctx.device)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    f = lib.lib.crychic_antialias
    assert f(ctx.handle, pa, pa, 64, 32, 0, 32, None, None) == -1 and "overlap" in lib.lib.crychic_last_error().decode()
    assert f(ctx.handle, None, pb, 64, 32, 0, 32, None, None) == -1
    assert f(ctx.handle, pa, pb, 0, 32, 0, 32, None, None) == -1
    assert f(ctx.handle, pa, pb, 64, 32, 1, 32, None, None) == -1
    bad = lib.AAParams(2048, 3, 17, 192)
    assert f(ctx.handle, pa, pb, 64, 32, 0, 32, C.byref(bad), None) == -1 and "searchSteps" in lib.lib.crychic_last_error().decode()
    torch.cuda.synchronize()
    assert bool((b == aa.GUARD).all()), "a refused call wrote"


@pytest.fixture(scope="module")
def app_frame(dev):
    """A Crychic over the 128 x 96 synthetic scene, and the frame Draw() gives without anti-aliasing."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    W, H, SD = 128, 96, 256
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 3, 3, LIGHT_SKY
    assert app.antiAliasing is None and app.mBackBufferAA is None
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.cpu().numpy().copy()
    assert app.mBackBufferAA is None
    return app, plain


def test_draw_with_anti_aliasing(dev, app_frame):
    lib, ctx, torch = dev
    from crychic_renderer_amd import AAParams
    app, plain = app_frame
    want, n = aa.checker(plain)
    assert n["horizontal"] + n["vertical"] > 0 and not np.array_equal(want, plain), "the scene has no edge to smooth"
    app.mBackBuffer.zero_()
    app.antiAliasing = True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "the back buffer differs from the Draw() without anti-aliasing"
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), want)
        # an AAParams: its values reach the pass
        app.antiAliasing = AAParams.default(searchSteps=3, subpix=0)
        app.Draw()
        torch.cuda.synchronize()
        want3, _ = aa.checker(plain, dict(searchSteps=3, subpix=0))
        assert not np.array_equal(want3, want) and np.array_equal(app.mBackBufferAA.cpu().numpy(), want3)
        # antialias() on its own: another destination, a row range
        out = torch.full_like(app.mBackBuffer, aa.GUARD)
        assert app.antialias(out=out, row0=7, rows=50) is out
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[7:57], want[7:57]) and (got[:7] == aa.GUARD).all() and (got[57:] == aa.GUARD).all()
    finally:
        app.antiAliasing = None


def test_strip_or_shared_draw_raises(dev, app_frame):
    lib, ctx, torch = dev
    app, plain = app_frame
    app.antiAliasing = True
    try:
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError):
                app.Draw(**kw)
        app.Draw(row0=0, rows=96)           # the whole frame, spelled out
    finally:
        app.antiAliasing = None
    app.Draw(row0=0, rows=48)               # without it a strip is a strip
    torch.cuda.synchronize()


def test_draw_and_pass_replay_from_a_graph(dev, app_frame):
    lib, ctx, torch = dev
    app, plain = app_frame
    want, _ = aa.checker(plain)
    app.antiAliasing = True
    try:
        app.Draw()                          # before the capture: mBackBufferAA allocated, the code objects loaded
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            app.Draw()
        for _ in range(2):
            app.mBackBuffer.zero_()
            app.mBackBufferAA.fill_(aa.GUARD)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
            assert np.array_equal(app.mBackBufferAA.cpu().numpy(), want)
    finally:
        app.antiAliasing = None
