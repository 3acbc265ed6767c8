"""crychic_sharpen on the device: the kernels against the checker (tests/sharpen_ref) on every byte -- the CPU tier's frames (below one
quad; widths around the quad, around what a wavefront and what a workgroup covers; heights around the strip a lane walks), every
4-byte misalignment of either plane, row ranges and known answers, behind guard bytes and with the input untouched; a second trip
with other parameters on the same context; and the refusals, with nothing written."""
import ctypes as C

import numpy as np
import pytest

import sharpen_lib as sl
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu


def run_device(dev, img, strength=256, limit=sl.DEFAULT_LIMIT, misalign=0, out_misalign=None, ranges=None, params=True):
    """crychic_sharpen on guarded device copies (the planes `misalign` / `out_misalign` bytes past a 256-byte boundary), over the whole
    frame or each (row0, rows) of `ranges`; params False: NULL, the defaults.  Returns the frame as numpy; guards and input checked."""
    lib, ctx, torch = dev
    H, W = img.shape[:2]
    planes = DevicePlanes(dev)
    src = planes.upload("input", img, misalign)
    out = planes.blank("out", img.shape, np.uint8, misalign if out_misalign is None else out_misalign)
    p = lib.SharpenParams.default(strength=strength, limit=limit)
    s = torch.cuda.current_stream(ctx.device)
    for row0, rows in ranges or [(0, H)]:
        lib.check(lib.lib.crychic_sharpen(ctx.handle, C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), W, H, row0, rows,
                                          C.byref(p) if params else None, C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return out.cpu().numpy().reshape(img.shape)


@pytest.mark.parametrize("kind", sl.KINDS)
def test_device_equals_checker(dev, kind):
    for W, H in sl.FRAMES:
        img = sl.frame(W, H, kind)
        for strength, limit in (sl.PARAMS[:2] if kind != "random" else sl.PARAMS):
            ref = sl.checker(img, strength, limit)
            got = run_device(dev, img, strength, limit)
            assert np.array_equal(got, ref), "%dx%d strength %d limit %d: %d bytes differ" % (W, H, strength, limit, int((got != ref).sum()))


@pytest.mark.parametrize("W,H", [(8, 3), (12, 2 * sl.STRIP + 1), (sl.WAVE_PIXELS + 4, 3), (7, 3)])
def test_misaligned_planes(dev, W, H):
    """`in` and `out` each 4, 8 and 12 bytes past a 16-byte boundary: the narrow kernel, never a refusal."""
    img = sl.frame(W, H, "smooth")
    ref = sl.checker(img)
    for mi in sl.MISALIGN:
        for mo in sl.MISALIGN:
            got = run_device(dev, img, misalign=mi, out_misalign=mo)
            assert np.array_equal(got, ref), "%dx%d, in %d and out %d bytes past a 16-byte boundary" % (W, H, mi, mo)


def test_known_answers(dev):
    from test_sharpen_host import answers
    answers(lambda img, s, l: run_device(dev, img, s, l))
    answers(lambda img, s, l: run_device(dev, img, s, l, misalign=12))


def test_null_params_are_the_defaults(dev):
    lib = dev[0]
    img = sl.frame(sl.WAVE_PIXELS + 4, 3, "smooth")
    d = lib.SharpenParams.default()
    assert np.array_equal(run_device(dev, img, params=False), sl.checker(img, d.strength, d.limit))


@pytest.mark.parametrize("W,H", [(12, 2 * sl.STRIP + 1), (13, 2 * sl.STRIP + 1), (sl.WAVE_PIXELS + 4, 3), (sl.GROUP_PIXELS + 4, 3), (5, 1), (1, 5)])
def test_row_ranges(dev, W, H):
    img = sl.frame(W, H, "smooth")
    ref = sl.checker(img)
    for row0, rows in sl.row_ranges(H):
        got = run_device(dev, img, ranges=[(row0, rows)])
        want = np.full_like(ref, sl.GUARD)
        want[row0:row0 + rows] = ref[row0:row0 + rows]
        assert np.array_equal(got, want), (W, H, row0, rows)
    assert (run_device(dev, img, ranges=[(0, 0)]) == sl.GUARD).all(), "rows == 0 wrote"
    for ranges in sl.stitches(H):
        assert np.array_equal(run_device(dev, img, ranges=ranges), ref), ranges


def test_second_trip_with_other_parameters(dev):
    """Two launches back to back on one stream into two planes, nothing between them: the second's parameters are its own."""
    lib, ctx, torch = dev
    img = sl.frame(sl.GROUP_PIXELS + 4, 3, "smooth")
    H, W = img.shape[:2]
    planes = DevicePlanes(dev)
    src = planes.upload("input", img)
    outs = [planes.blank("out %d" % k, img.shape) for k in range(3)]
    sets = ((256, 3584), (32, 1000), (256, 3584))
    s = torch.cuda.current_stream(ctx.device)
    for (strength, limit), out in zip(sets, outs):
        p = lib.SharpenParams.default(strength=strength, limit=limit)
        lib.check(lib.lib.crychic_sharpen(ctx.handle, C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), W, H, 0, H, C.byref(p), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    for (strength, limit), out in zip(sets, outs):
        assert np.array_equal(out.cpu().numpy().reshape(img.shape), sl.checker(img, strength, limit)), (strength, limit)
    assert not np.array_equal(sl.checker(img, 256, 3584), sl.checker(img, 32, 1000))


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    W, H = 64, 32
    a = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((H * W * 4 + 16,), sl.GUARD, dtype=torch.uint8, device=ctx.device)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    f, err = lib.lib.crychic_sharpen, lib.lib.crychic_last_error
    bad = lib.SharpenParams.default(strength=257)
    assert f(ctx.handle, pa, pb, W, H, 0, H, C.byref(bad), None) == -1 and "strength" in err().decode()
    bad = lib.SharpenParams.default(limit=3585)
    assert f(ctx.handle, pa, pb, W, H, 0, H, C.byref(bad), None) == -1 and "limit" in err().decode()
    bad = lib.SharpenParams.default()
    bad.reserved[0] = 7
    assert f(ctx.handle, pa, pb, W, H, 0, H, C.byref(bad), None) == -1 and "reserved" in err().decode()
    assert f(ctx.handle, None, pb, W, H, 0, H, None, None) == -1 and f(ctx.handle, pa, None, W, H, 0, H, None, None) == -1
    assert f(ctx.handle, pa, pb, W, H, 2, H - 1, None, None) == -1 and "rows" in err().decode()
    assert f(ctx.handle, pa, pa, W, H, 0, H, None, None) == -1 and "overlap" in err().decode()
    assert f(ctx.handle, pa, C.c_void_p(a.data_ptr() + 4), W, H, 0, H - 1, None, None) == -1 and "overlap" in err().decode()
    assert f(ctx.handle, pa, C.c_void_p(b.data_ptr() + 2), W, H, 0, H, None, None) == -1 and "aligned" in err().decode()
    assert f(ctx.handle, pa, pb, 0, H, 0, 0, None, None) == -1
    assert f(ctx.handle, pa, pb, 1 << 15, (1 << 13) + 1, 0, 1, None, None) == -4
    assert f(None, pa, pb, W, H, 0, H, None, None) == -1 and "null context" in err().decode()
    torch.cuda.synchronize()
    assert (b == sl.GUARD).all(), "a refused call wrote"
