"""crychic_dof on the device: the kernel against the checker (tests/dof_ref) byte for byte on the corpus of the CPU tier, behind guard
bytes, on misaligned planes and in row ranges; the known answers; and the pass behind Crychic.Draw -- alone, behind the fog and in
front of the anti-aliasing, and replayed from a graph."""
import ctypes as C

import numpy as np
import pytest

import dof_lib as dl
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu


def run_device(dev, frame, img, params=None, row0=0, rows=None, misalign=0):
    """crychic_dof on guarded device copies of `img` and the depth plane; returns the output plane as numpy, the guards and the inputs
    checked."""
    lib, ctx, torch = dev
    H, W = img.shape[:2]
    planes = DevicePlanes(dev)
    src = planes.upload("input", img, misalign)
    depth = planes.upload("depth", frame.depth, misalign)
    out = planes.blank("out", img.shape, np.uint8, misalign)
    pcb = frame.pass_constants(lib)
    p = None
    if params is not None:
        q = dict(dl.DEFAULTS, **params)
        p = lib.DofParams.default(focus=q["focus"], aperture=q["aperture"], radius=q["radius"])
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_dof(ctx.handle, C.byref(pcb), C.c_void_p(depth.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), W, H,
                                  row0, H - row0 if rows is None else rows, None if p is None else C.byref(p), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return out.cpu().numpy().reshape(img.shape)


@pytest.mark.parametrize("pname", list(dl.PARAM_SETS))
def test_device_equals_checker(dev, pname):
    turn = 0
    for name, frame, img, pn, _ in dl.corpus():
        if pn != pname:
            continue
        ref, _ = dl.expected(name)
        got = run_device(dev, frame, img, None if pn == "default" else dl.PARAM_SETS[pn])
        assert np.array_equal(got, ref), "%s: %d bytes differ" % (name, int((got != ref).sum()))
        misalign = (4, 12)[turn % 2]
        turn += 1
        got = run_device(dev, frame, img, dl.PARAM_SETS[pn], misalign=misalign)
        assert np.array_equal(got, ref), "%s, planes %d bytes past a 16-byte boundary: %d bytes differ" % (name, misalign, int((got != ref).sum()))


def test_known_answers(dev):
    from test_dof_host import answers
    answers(lambda f, i, p: run_device(dev, f, i, p))
    answers(lambda f, i, p: run_device(dev, f, i, p, misalign=12))


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 96, 101, 190), (0, 16, 31, 189, 190)])
def test_row_ranges_stitch_to_the_whole_frame(dev, split):
    by_name = {c[0]: c for c in dl.corpus()}
    for name, misalign in ((dl.case_name("322x190_random"), 0), ("322x190_step_near_blurred", 4)):
        _, frame, img, pn, _ = by_name[name]
        whole, _ = dl.expected(name)
        stitched = np.full(img.shape, dl.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got = run_device(dev, frame, img, dl.PARAM_SETS[pn], row0=row0, rows=end - row0, misalign=misalign)
            assert (got[:row0] == dl.GUARD).all() and (got[end:] == dl.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
        assert np.array_equal(stitched, whole), name
    _, frame, img, _, _ = by_name["scene128_default"]
    assert (run_device(dev, frame, img, None, row0=96, rows=0) == dl.GUARD).all(), "rows == 0 wrote"


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    a = torch.zeros((32, 64, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((32, 65, 4), dl.GUARD, dtype=torch.uint8, device=ctx.device)
    d = torch.zeros((32, 64), dtype=torch.int32, device=ctx.device)
    pa, pb, pd = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(d.data_ptr())
    cb = dl.Frame(dl.REFERENCE_AB, np.zeros((1, 1), np.uint32)).pass_constants(lib)
    f = lib.lib.crychic_dof
    assert f(ctx.handle, C.byref(cb), pd, pa, pa, 64, 32, 0, 32, None, None) == -1 and "overlap" in lib.lib.crychic_last_error().decode()
    assert f(ctx.handle, C.byref(cb), pd, pa, C.c_void_p(a.data_ptr() + 4), 64, 32, 0, 32, None, None) == -1
    assert f(ctx.handle, C.byref(cb), pd, None, pb, 64, 32, 0, 32, None, None) == -1
    assert f(ctx.handle, C.byref(cb), pd, pa, pb, 64, 32, 1, 32, None, None) == -1
    bad = lib.DofParams.default(radius=9)
    assert f(ctx.handle, C.byref(cb), pd, pa, pb, 64, 32, 0, 32, C.byref(bad), None) == -1 and "maxRadius" in lib.lib.crychic_last_error().decode()
    cb.Proj[11] = 0.0
    assert f(ctx.handle, C.byref(cb), pd, pa, pb, 64, 32, 0, 32, None, None) == -1 and "Proj[11]" in lib.lib.crychic_last_error().decode()
    torch.cuda.synchronize()
    assert bool((b == dl.GUARD).all()), "a refused call wrote"


@pytest.fixture(scope="module")
def app_frame(dev):
    """A Crychic over the 128 x 96 synthetic scene, the frame Draw() gives without the pass, and what the passes read of the scene."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    import fog_lib as fg
    W, H, SD = 128, 96, 256
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 3, 3, LIGHT_SKY
    assert app.depthOfField is None and app.mBackBufferDoF is None
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.cpu().numpy().copy()
    depth = planes["depth"].cpu().numpy().view(np.uint32)
    frame = dl.Frame.from_pass_cb(app.mMainPassCB, depth)
    fog_frame = fg.Frame.from_pass_cb(app.mMainPassCB, depth, planes["shadow"].cpu().numpy().view(np.uint32))
    return app, plain, frame, fog_frame


def test_draw_with_depth_of_field(dev, app_frame):
    lib, ctx, torch = dev
    from crychic_renderer_amd import DofParams
    app, plain, frame, _ = app_frame
    want, n = dl.checker(frame, plain)
    assert n["k_interior"] > 0 and n["behind"] > 0 and not np.array_equal(want, plain), "the scene is all in focus"
    app.depthOfField = True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferDoF.cpu().numpy(), want), "mBackBufferDoF is not the checker's frame over mBackBuffer"
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "mBackBuffer is not the frame of the Draw() without the switch"
        # a DofParams: its values reach the pass
        app.depthOfField = DofParams.default(focus=30.0, aperture=20.0, radius=5)
        app.Draw()
        torch.cuda.synchronize()
        want5, _ = dl.checker(frame, plain, dict(focus=30.0, aperture=20.0, radius=5))
        assert not np.array_equal(want5, want) and np.array_equal(app.mBackBufferDoF.cpu().numpy(), want5)
    finally:
        app.depthOfField = None
    # set and cleared: Draw() issues what it issued before the attribute was ever set
    app.mBackBuffer.zero_()
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "with depthOfField unset Draw() gives the frame it gave before"
    assert np.array_equal(app.mBackBufferDoF.cpu().numpy(), want5), "with depthOfField unset Draw() still wrote mBackBufferDoF"
    # depth_of_field on its own: another destination and a row range; mBackBuffer stays
    out = torch.full_like(app.mBackBuffer, dl.GUARD)
    assert app.depth_of_field(out=out, row0=7, rows=50) is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[7:57], want[7:57]) and (got[:7] == dl.GUARD).all() and (got[57:] == dl.GUARD).all()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
    assert app.depth_of_field() is app.mBackBufferDoF
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBufferDoF.cpu().numpy(), want)
    with pytest.raises(lib.CrychicError):
        app.depth_of_field(out=app.mBackBuffer)            # in place is refused


def test_fog_then_depth_of_field_then_anti_aliasing(dev, app_frame):
    lib, ctx, torch = dev
    import fog_lib as fg
    import post_aa_lib as aa
    app, plain, frame, fog_frame = app_frame
    fogged, _ = fg.checker(fog_frame, plain)
    blurred, _ = dl.checker(frame, fogged)
    want, n = aa.checker(blurred)
    assert not np.array_equal(fogged, plain) and not np.array_equal(blurred, fogged) and not np.array_equal(want, blurred)
    app.fog, app.depthOfField, app.antiAliasing = True, True, True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), fogged)
        assert np.array_equal(app.mBackBufferDoF.cpu().numpy(), blurred)
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), want), "mBackBufferAA is not AA-checker(DoF-checker(fog-checker(plain frame)))"
        assert app.fog is True and app.depthOfField is True and app.antiAliasing is True
        # without the fog: the anti-aliasing reads mBackBufferDoF
        app.fog = None
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), aa.checker(dl.checker(frame, plain)[0])[0])
    finally:
        app.fog, app.depthOfField, app.antiAliasing = None, None, None
    # the fog and the anti-aliasing without the pass: as before it existed
    app.fog, app.antiAliasing = True, True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), aa.checker(fogged)[0])
    finally:
        app.fog, app.antiAliasing = None, None


def test_strip_or_shared_draw_raises(dev, app_frame):
    lib, ctx, torch = dev
    app = app_frame[0]
    app.depthOfField = True
    try:
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError):
                app.Draw(**kw)
        app.Draw(row0=0, rows=96)           # the whole frame, spelled out
    finally:
        app.depthOfField = None
    app.Draw(row0=0, rows=48)               # without it a strip is a strip
    torch.cuda.synchronize()


def test_draw_and_pass_replay_from_a_graph(dev, app_frame):
    lib, ctx, torch = dev
    app, plain, frame, _ = app_frame
    want, _ = dl.checker(frame, plain)
    app.depthOfField = True
    try:
        app.Draw()                          # before the capture: the code objects loaded, mBackBufferDoF allocated
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            app.Draw()
        for _ in range(2):
            app.mBackBuffer.zero_()
            app.mBackBufferDoF.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
            assert np.array_equal(app.mBackBufferDoF.cpu().numpy(), want)
    finally:
        app.depthOfField = None
