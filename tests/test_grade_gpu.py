"""crychic_grade on the device: the kernel against the checker (tests/grade_ref) on every byte -- the CPU tier's frames, misalignments,
row ranges and known answers, behind guard bytes and with the inputs untouched; a frame that gives some workgroup a second trip
whatever the grid; the frame of every RGB triple; and tables of different sizes back to back on one stream."""
import ctypes as C

import numpy as np
import pytest

import grade_lib as gl
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu


def run_device(dev, img, lut, misalign=0, out_misalign=None, in_place=False, ranges=None, lut_misalign=0):
    """crychic_grade on guarded device copies of `img` and `lut` (the planes `misalign` / `out_misalign` bytes past a 256-byte
    boundary), over the whole frame or each (row0, rows) of `ranges`.  Returns the frame as numpy; the guards and the inputs checked."""
    lib, ctx, torch = dev
    H, W = img.shape[:2]
    planes = DevicePlanes(dev)
    src = planes.upload("input", img, misalign, writable=in_place)
    out = src if in_place else planes.blank("out", img.shape, np.uint8, misalign if out_misalign is None else out_misalign)
    table = planes.upload("table", np.ascontiguousarray(lut), lut_misalign)
    s = torch.cuda.current_stream(ctx.device)
    for row0, rows in ranges or [(0, H)]:
        lib.check(lib.lib.crychic_grade(ctx.handle, C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), W, H, row0, rows,
                                        C.c_void_p(table.data_ptr()), lut.shape[0], C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return out.cpu().numpy().reshape(img.shape)


@pytest.mark.parametrize("N", gl.SIZES)
def test_device_equals_checker(dev, N):
    lut = gl.corpus_lut(N)
    for W, H in gl.FRAMES:
        img = gl.frame(W, H)
        ref = gl.checker(img, lut)
        for misalign in gl.MISALIGN:
            got = run_device(dev, img, lut, misalign=misalign, lut_misalign=4 * (misalign // 4 % 2))
            assert np.array_equal(got, ref), "%dx%d, %d bytes past a 16-byte boundary: %d bytes differ" % (W, H, misalign, int((got != ref).sum()))
        got = run_device(dev, img, lut, misalign=8, in_place=True)
        assert np.array_equal(got, ref), "%dx%d in place" % (W, H)
        got = run_device(dev, img, lut, misalign=4, out_misalign=8)          # aligned differently: the narrow path
        assert np.array_equal(got, ref), "%dx%d, planes aligned differently" % (W, H)
    tie = gl.tie_frame(N)
    assert np.array_equal(run_device(dev, tie, lut), gl.checker(tie, lut)), "the tie frame"


def test_known_answers(dev):
    from test_grade_host import answers
    answers(lambda img, lut: run_device(dev, img, lut))
    answers(lambda img, lut: run_device(dev, img, lut, misalign=12))


@pytest.mark.parametrize("W,H", [(67, 5), (5, 3), (3, 1)])
def test_row_ranges(dev, W, H):
    img, lut = gl.frame(W, H), gl.corpus_lut(33)
    ref = gl.checker(img, lut)
    for row0, rows in gl.row_ranges(H):
        for misalign in (0, 4):
            got = run_device(dev, img, lut, misalign=misalign, ranges=[(row0, rows)])
            want = np.full_like(ref, gl.GUARD)
            want[row0:row0 + rows] = ref[row0:row0 + rows]
            assert np.array_equal(got, want), (W, H, row0, rows, misalign)
    assert (run_device(dev, img, lut, ranges=[(0, 0)]) == gl.GUARD).all(), "rows == 0 wrote"
    assert np.array_equal(run_device(dev, img, lut, ranges=[(r, 1) for r in range(H)]), ref), "single rows do not stitch to the frame"


@pytest.mark.parametrize("N", (17, 33))
def test_second_trip(dev, N):
    """1024 x 1100 = 1.13 M texels: more than 256 compute units x 1024 lanes x 4 texels, so some workgroup strides on."""
    img = np.random.default_rng(11).integers(0, 256, (1100, 1024, 4), dtype=np.uint8)
    lut = gl.corpus_lut(N)
    ref = gl.checker(img, lut)
    assert np.array_equal(run_device(dev, img, lut), ref)
    assert np.array_equal(run_device(dev, img, lut, misalign=12, in_place=True), ref)


_EVERY = {}


def every_triple():
    """4096 x 4096: every (R, G, B) once, alpha from the low bits; built once, read-only."""
    if "img" not in _EVERY:
        t = np.arange(1 << 24, dtype=np.uint32)
        img = (t | ((t * np.uint32(2654435761)) & np.uint32(0xFF000000))).view(np.uint8).reshape(4096, 4096, 4)
        img.setflags(write=False)
        _EVERY["img"] = img
    return _EVERY["img"]


@pytest.mark.parametrize("N", (33, 17))
def test_every_rgb_triple(dev, N):
    lib, ctx, torch = dev
    img, lut = every_triple(), gl.corpus_lut(N)
    got = run_device(dev, img, lut)
    ref = gl.checker(img, lut)
    assert np.array_equal(got, ref), "%d bytes differ" % int((got != ref).sum())


def test_tables_back_to_back(dev):
    """Sizes 2, 16, 17, 33 and back down on one stream with nothing between the launches: a stale LDS size or a stale fill would show."""
    lib, ctx, torch = dev
    img = gl.frame(128, 96)
    H, W = img.shape[:2]
    order = (2, 16, 17, 33, 17, 2, 33, 16)
    planes = DevicePlanes(dev)
    src = planes.upload("input", img)
    tables = {N: planes.upload("table %d" % N, gl.corpus_lut(N)) for N in set(order)}
    outs = [planes.blank("out %d" % k, img.shape) for k in range(len(order))]
    s = torch.cuda.current_stream(ctx.device)
    for N, out in zip(order, outs):
        lib.check(lib.lib.crychic_grade(ctx.handle, C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), W, H, 0, H,
                                        C.c_void_p(tables[N].data_ptr()), N, C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    for N, out in zip(order, outs):
        assert np.array_equal(out.cpu().numpy().reshape(img.shape), gl.checker(img, gl.corpus_lut(N))), N


def test_refusals_with_a_context(dev):
    lib, ctx, torch = dev
    W, H = 64, 32
    a = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    b = torch.full((H, W, 4), gl.GUARD, dtype=torch.uint8, device=ctx.device)
    t = torch.zeros((4 * 33 ** 3 + 16,), dtype=torch.uint8, device=ctx.device)
    pa, pb, pt = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(t.data_ptr())
    f, err = lib.lib.crychic_grade, lib.lib.crychic_last_error
    assert f(ctx.handle, pa, pb, W, H, 0, H, pt, 1, None) == -1 and f(ctx.handle, pa, pb, W, H, 0, H, pt, 34, None) == -1
    assert f(ctx.handle, None, pb, W, H, 0, H, pt, 17, None) == -1 and f(ctx.handle, pa, pb, W, H, 0, H, None, 17, None) == -1
    assert f(ctx.handle, pa, pb, W, H, 2, H - 1, pt, 17, None) == -1 and "rows" in err().decode()
    assert f(ctx.handle, pa, C.c_void_p(a.data_ptr() + 4), W, H, 0, H - 1, pt, 17, None) == -1 and "overlap" in err().decode()
    assert f(ctx.handle, pa, pb, W, H, 0, H, C.c_void_p(t.data_ptr() + 2), 17, None) == -1 and "aligned" in err().decode()
    assert f(None, pa, pb, W, H, 0, H, pt, 17, None) == -1 and "null context" in err().decode()
    torch.cuda.synchronize()
    assert (b == gl.GUARD).all(), "a refused call wrote"
