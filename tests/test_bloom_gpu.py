"""crychic_bloom on the device: the kernels against the checker (tests/bloom_ref) byte for byte on the corpus of the CPU tier -- the
frame and every level of the workspace, so that a difference names its kernel -- behind guard bytes, on misaligned planes, in place and
in row ranges; the known answers; the refusals; and the pass behind Crychic.Draw -- alone, behind the fog and the depth of field and
in front of the anti-aliasing, set and cleared, and replayed from a graph."""
import ctypes as C

import numpy as np
import pytest

import bloom_lib as bl
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu


def bloom_params(lib, params):
    return None if params is None else lib.BloomParams.default(**dict(bl.DEFAULTS, **params))


def run_device(dev, img, params=None, misalign=0, in_place=False, split=None, ws_misalign=0):
    """crychic_bloom on guarded device copies of `img` and a guarded workspace of 0xA5 (16 * ws_misalign bytes past a 256-byte
    boundary); with `split`, crychic_bloom_pyramid and then crychic_bloom_composite over each row range.  Returns (frame, [U_k]) as
    numpy, the guards, the input and the workspace's gaps checked."""
    lib, ctx, torch = dev
    H, W = img.shape[:2]
    p = dict(bl.DEFAULTS, **(params or {}))
    _, need = bl.level_offsets(W, H, p["levels"])
    planes = DevicePlanes(dev)
    src = planes.upload("input", img, misalign, writable=in_place)
    out = src if in_place else planes.blank("out", img.shape, np.uint8, misalign)
    ws = planes.blank("workspace", need, np.uint8, 16 * ws_misalign)
    q = bloom_params(lib, params)
    qp = None if q is None else C.byref(q)
    s = torch.cuda.current_stream(ctx.device)
    stream = C.c_void_p(s.cuda_stream)
    ps, po, pw = C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr())
    if split is None:
        lib.check(lib.lib.crychic_bloom(ctx.handle, ps, po, W, H, qp, pw, need, stream))
    else:
        lib.check(lib.lib.crychic_bloom_pyramid(ctx.handle, ps, W, H, qp, pw, need, stream))
        for row0, end in zip(split[:-1], split[1:]):
            lib.check(lib.lib.crychic_bloom_composite(ctx.handle, ps, po, W, H, row0, end - row0, qp, pw, need, stream))
    s.synchronize()
    planes.verify()
    wsh = ws.cpu().numpy()
    assert (wsh[~bl.written_mask(W, H, p["levels"], need)] == bl.GUARD).all(), "a workspace byte between two levels was written"
    return out.cpu().numpy().reshape(img.shape), bl.split_workspace(wsh, W, H, p["levels"])


def assert_equal(name, got, levels, ref, ref_levels):
    assert len(levels) == len(ref_levels), name
    for k, (g, r) in enumerate(zip(levels, ref_levels), 1):
        assert np.array_equal(g, r), "%s: level %d differs in %d values" % (name, k, int((g != r).sum()))
    assert np.array_equal(got, ref), "%s: %d bytes of the frame differ" % (name, int((got != ref).sum()))


@pytest.mark.parametrize("pname", list(bl.PARAM_SETS) + ["scene"])
def test_device_equals_checker(dev, pname):
    turn = 0
    for name, img, pn in bl.corpus():
        if pn != pname:
            continue
        ref, ref_levels, _ = bl.expected(name)
        prm = None if pn == "default" else bl.case_params(pn)
        got, levels = run_device(dev, img, prm)
        assert_equal(name, got, levels, ref, ref_levels)
        misalign = (4, 12)[turn % 2]
        turn += 1
        got, levels = run_device(dev, img, bl.case_params(pn), misalign=misalign, ws_misalign=turn % 3)
        assert_equal("%s, planes %d bytes past a 16-byte boundary" % (name, misalign), got, levels, ref, ref_levels)
        got, levels = run_device(dev, img, bl.case_params(pn), misalign=(0, 8)[turn % 2], in_place=True)
        assert_equal(name + " in place", got, levels, ref, ref_levels)


def test_known_answers(dev):
    from test_bloom_host import answers
    answers(lambda img, p: run_device(dev, img, p))
    answers(lambda img, p: run_device(dev, img, p, misalign=12))


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 96, 101, 190)])
def test_row_ranges_stitch_to_the_whole_frame(dev, split):
    name = "322x190_blob_default"
    img = {c[0]: c for c in bl.corpus()}[name][1]
    ref, ref_levels, _ = bl.expected(name)
    for misalign in (0, 4):
        got, levels = run_device(dev, img, None, misalign=misalign, split=split)
        assert_equal(name, got, levels, ref, ref_levels)
    # one range alone leaves the other rows as they were
    got, _ = run_device(dev, img, None, split=(split[1], split[2]))
    assert (got[:split[1]] == bl.GUARD).all() and (got[split[2]:] == bl.GUARD).all() and np.array_equal(got[split[1]:split[2]], ref[split[1]:split[2]])
    got, _ = run_device(dev, img, None, split=(190, 190))
    assert (got == bl.GUARD).all(), "rows == 0 wrote"


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    W, H = 64, 32
    need = bl.level_offsets(W, H, 6)[1]
    a = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((H, W + 1, 4), bl.GUARD, dtype=torch.uint8, device=ctx.device)
    w = torch.full((need + 64,), bl.GUARD, dtype=torch.uint8, device=ctx.device)
    pa, pb, pw = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(w.data_ptr())
    f, fp, fc, err = lib.lib.crychic_bloom, lib.lib.crychic_bloom_pyramid, lib.lib.crychic_bloom_composite, lib.lib.crychic_last_error
    assert f(ctx.handle, pa, C.c_void_p(a.data_ptr() + 4), W, H, None, pw, need, None) == -1 and "overlap" in err().decode()
    assert f(ctx.handle, pa, pb, W, H, None, pw, need - 1, None) == -1 and "workspace has" in err().decode()
    assert f(ctx.handle, pa, pb, W, H, None, C.c_void_p(w.data_ptr() + 8), need, None) == -1 and "16-byte" in err().decode()
    assert f(ctx.handle, pa, pb, W, H, None, pb, need, None) == -1 and "workspace overlaps" in err().decode()
    assert f(ctx.handle, None, pb, W, H, None, pw, need, None) == -1
    bad = lib.BloomParams.default(levels=9)
    assert f(ctx.handle, pa, pb, W, H, C.byref(bad), pw, need, None) == -1 and "levels" in err().decode()
    assert fp(ctx.handle, pa, W, H, C.byref(bad), pw, need, None) == -1 and fp(ctx.handle, pa, W, 0, None, pw, need, None) == -1
    assert fc(ctx.handle, pa, pb, W, H, 1, H, None, pw, need, None) == -1 and "outside" in err().decode()
    bad = lib.BloomParams.default(knee=0)
    assert fc(ctx.handle, pa, pb, W, H, 0, H, C.byref(bad), pw, need, None) == -1 and "knee" in err().decode()
    torch.cuda.synchronize()
    assert bool((b == bl.GUARD).all()) and bool((w == bl.GUARD).all()) and not bool(a.any()), "a refused call wrote"


@pytest.fixture(scope="module")
def app_frame(dev):
    """A Crychic over the 128 x 96 synthetic scene, the frame Draw() gives without the pass, and what the other passes read."""
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    import dof_lib as dl
    import fog_lib as fg
    W, H, SD = 128, 96, 256
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 3, 3, LIGHT_SKY
    assert app.bloom is None and app.mBackBufferBloom is None and app.mBloomWorkspace is None
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.cpu().numpy().copy()
    depth = planes["depth"].cpu().numpy().view(np.uint32)
    dof_frame = dl.Frame.from_pass_cb(app.mMainPassCB, depth)
    fog_frame = fg.Frame.from_pass_cb(app.mMainPassCB, depth, planes["shadow"].cpu().numpy().view(np.uint32))
    return app, plain, dof_frame, fog_frame


def scene_params(lib):
    return lib.BloomParams.default(**bl.SCENE_PARAMS)


def test_draw_with_bloom(dev, app_frame):
    lib, ctx, torch = dev
    app, plain, _, _ = app_frame
    want, levels, n = bl.checker(plain, bl.SCENE_PARAMS)
    assert n["w_interior"] + n["w_full"] > 0 and not np.array_equal(want, plain), "nothing of the scene lies over the threshold"
    app.bloom = scene_params(lib)
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferBloom.cpu().numpy(), want), "mBackBufferBloom is not the checker's frame over mBackBuffer"
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "mBackBuffer is not the frame of the Draw() without the switch"
        got = bl.split_workspace(app.mBloomWorkspace.cpu().numpy(), 128, 96, 6)
        assert all(np.array_equal(g, u) for g, u in zip(got, levels)), "mBloomWorkspace does not hold the checker's levels"
        # True: the defaults
        app.bloom = True
        app.Draw()
        torch.cuda.synchronize()
        at_defaults = bl.checker(plain)[0]
        assert not np.array_equal(at_defaults, plain) and not np.array_equal(at_defaults, want), "nothing of the scene lies over luma 192"
        assert np.array_equal(app.mBackBufferBloom.cpu().numpy(), at_defaults)
        app.bloom = scene_params(lib)
        app.Draw()
        torch.cuda.synchronize()
    finally:
        app.bloom = None
    # set and cleared: Draw() issues what it issued before the attribute was ever set
    app.mBackBuffer.zero_()
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain), "with bloom unset Draw() gives the frame it gave before"
    assert np.array_equal(app.mBackBufferBloom.cpu().numpy(), want), "with bloom unset Draw() still wrote mBackBufferBloom"
    # apply_bloom on its own: another destination, in place on a copy, and the defaults of its arguments
    out = torch.full_like(app.mBackBuffer, bl.GUARD)
    assert app.apply_bloom(out=out, params=scene_params(lib)) is out
    copy = app.mBackBuffer.clone()
    assert app.apply_bloom(src=copy, out=copy, params=scene_params(lib)) is copy
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(copy.cpu().numpy(), want)
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
    assert app.apply_bloom() is app.mBackBufferBloom
    with pytest.raises(lib.CrychicError):
        app.apply_bloom(out=torch.zeros((96, 64, 4), dtype=torch.uint8, device=ctx.device))


def test_fog_then_depth_of_field_then_bloom_then_anti_aliasing(dev, app_frame):
    lib, ctx, torch = dev
    import dof_lib as dl
    import fog_lib as fg
    import post_aa_lib as aa
    app, plain, dof_frame, fog_frame = app_frame
    fogged, _ = fg.checker(fog_frame, plain)
    blurred, _ = dl.checker(dof_frame, fogged)
    bloomed = bl.checker(blurred, bl.SCENE_PARAMS)[0]
    want, _ = aa.checker(bloomed)
    assert not np.array_equal(fogged, plain) and not np.array_equal(blurred, fogged) and not np.array_equal(bloomed, blurred) and not np.array_equal(want, bloomed)
    app.fog, app.depthOfField, app.bloom, app.antiAliasing = True, True, scene_params(lib), True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), fogged)
        assert np.array_equal(app.mBackBufferDoF.cpu().numpy(), blurred)
        assert np.array_equal(app.mBackBufferBloom.cpu().numpy(), bloomed)
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), want), "mBackBufferAA is not AA(bloom(DoF(fog(plain frame)))) of the checkers"
        assert app.fog is True and app.depthOfField is True and app.antiAliasing is True and isinstance(app.bloom, lib.BloomParams)
        # without the depth of field: the pass reads mBackBuffer, the anti-aliasing mBackBufferBloom
        app.depthOfField = None
        app.Draw()
        torch.cuda.synchronize()
        direct = bl.checker(fogged, bl.SCENE_PARAMS)[0]
        assert np.array_equal(app.mBackBufferBloom.cpu().numpy(), direct)
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), aa.checker(direct)[0])
    finally:
        app.fog, app.depthOfField, app.bloom, app.antiAliasing = None, None, None, None
    # the other passes without this one: as before it existed
    app.fog, app.depthOfField, app.antiAliasing = True, True, True
    try:
        app.Draw()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBufferAA.cpu().numpy(), aa.checker(blurred)[0])
        assert np.array_equal(app.mBackBufferBloom.cpu().numpy(), direct), "with bloom unset Draw() still wrote mBackBufferBloom"
    finally:
        app.fog, app.depthOfField, app.antiAliasing = None, None, None


def test_strip_or_shared_draw_raises(dev, app_frame):
    lib, ctx, torch = dev
    app = app_frame[0]
    app.bloom = True
    try:
        for kw in (dict(row0=0, rows=48), dict(row0=48), dict(shared=(None, None, 1))):
            with pytest.raises(lib.CrychicError):
                app.Draw(**kw)
        app.Draw(row0=0, rows=96)           # the whole frame, spelled out
    finally:
        app.bloom = None
    app.Draw(row0=0, rows=48)               # without it a strip is a strip
    torch.cuda.synchronize()


def test_draw_replays_from_a_graph(dev, app_frame):
    lib, ctx, torch = dev
    app, plain, _, _ = app_frame
    want = bl.checker(plain, bl.SCENE_PARAMS)[0]
    app.bloom = scene_params(lib)
    try:
        app.Draw()                          # before the capture: the code objects loaded, the buffer and the workspace allocated
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            app.Draw()
        for _ in range(2):
            app.mBackBuffer.zero_()
            app.mBackBufferBloom.zero_()
            app.mBloomWorkspace.fill_(bl.GUARD)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)
            assert np.array_equal(app.mBackBufferBloom.cpu().numpy(), want)
    finally:
        app.bloom = None
