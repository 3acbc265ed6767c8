"""ssao_kernel's prologue -- one batch of loads (centre, random-vector texels, geometry-map cell, border texels), edge-workspace
stores from the centre's own value, the sky shortcut's cells dealt one per lane -- on the device against the CPU oracle, bit for
bit, through the C ABI as tests/test_gpu_parity.py::test_ssao_bit_exact does.

Shapes, the smallest at which the changed code can go wrong:
  * 140 x 24: half-res width 70, so the second wavefront of a row has 6 live lanes and n < 64 in the cell sharing.  The frame is one
    cell row of the geometry map (32 texel rows) and every wavefront reaches both of its cell columns (the reach is at least 8
    texels), so a 140 x 24 frame with any geometry in it has NO wavefront that takes the shortcut: the sky-over-geometry frame of
    this size has refused and lit wavefronts only, and an all-sky frame of the same size takes the shortcut with n = 6.
  * 322 x 190: three wavefronts per row (the last with 33 live lanes), 3 x 6 cells; sky over geometry with the horizon inside the
    frame gives all three kinds of wavefront -- asserted on the CPU with the host build of the shortcut's predicate
    (tests/hostsim/ssao_prologue_host.cpp), so that the oracle alone decides whether the frames are honest.
  * 512 x 416 with OcclusionRadius 6.4: the reach covers the frame, whose 5 x 13 = 65 cells are the smallest whole-frame rectangle
    above 64 cells (a cell is 128 x 32 texels), so the kernel's fallback loop runs.
Runs: the whole frame, and two strips with row0 > 0 (both border copies, x == 0 and y == row0, run in each).  The sky shortcut and
the tap culling each on and off.  Compared: the ambient plane after crychic_ssao; the ambient plane after one blur iteration
(horizontal, then vertical sweep) over the same workspace, which reads edge.nrm, edge.vz, gcol and grow; for the strips the
horizontal sweep over the strip's rows, and the workspace's nrm / vz / gcol rows and grow against the host build's."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import ssao_prologue_lib as spl

SIZES = [(140, 24), (322, 190)]
SWITCHES = [(True, True), (False, True), (True, False), (False, False)]      # (sky shortcut, tap culling)
STRIPS = {(140, 24): ((3, 4), (8, 4)), (322, 190): ((31, 17), (72, 23))}

_frames = {}


def frame(W, H, sky, cull, kind="horizon"):
    """(constants, oracle constants, depth, normal, randvec, oracle SSAO plane) of one frame, computed once."""
    key = (W, H, sky, cull, kind)
    if key not in _frames:
        c = spl.constants(W, H, sky, cull, radius=6.4 if kind.startswith("wide") else None)
        depth, normal, randvec = spl.sky_over_geometry(c.ssao_cb, W, H, seed=W + H, horizon=H if kind in ("allsky", "wide-allsky") else
                                                       (H - 40) | 1 if kind == "wide-patch" else None)
        scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
        ref = oracle_lib.load().ssao(scb, normal, depth, randvec)
        _frames[key] = (c, scb, depth, normal, randvec, ref)
    return _frames[key]


# ---- CPU tier: the frames are honest, the lane mapping is the division ---------------------------------------------------------

def test_cell_of_lane_is_the_division(built_lib):
    """ssao_sky_cell_of_lane (reciprocal, no integer division) == row-major division for every rectangle of at most 64 cells."""
    assert spl.load().sp_cell_of_lane_mismatches() == 0


@pytest.mark.parametrize("sky,cull", SWITCHES)
def test_frames_hold_every_kind_of_wavefront(built_lib, sky, cull):
    """Counted on the CPU with the host build of the predicate: every 322 x 190 sky-over-geometry frame has wavefronts that take
    the shortcut (when the constants enable it), all-sky wavefronts that are refused, and lit ones -- whole frame and strips
    together; 140 x 24 has refused and lit ones, and its all-sky twin takes the shortcut on the 6-lane wavefronts too."""
    c, scb, depth, normal, randvec, ref = frame(322, 190, sky, cull)
    k = spl.classify(c.ssao_cb, normal, depth)
    assert (k["sky_enabled"], k["cull_enabled"]) == (int(sky), int(cull))
    assert k["refused"] > 0 and k["lit"] > 0 and k["lane_mismatches"] == 0
    assert (k["taken"] > 0) == sky
    assert ref.min() < 65535 and (ref == 65535).any()
    for row0, rows in STRIPS[(322, 190)]:
        ks = spl.classify(c.ssao_cb, normal, depth, row0, rows)
        assert ks["refused"] + ks["taken"] > 0 or ks["lit"] > 0
    c, scb, depth, normal, randvec, ref = frame(140, 24, sky, cull)
    k = spl.classify(c.ssao_cb, normal, depth)
    assert k["taken"] == 0 and k["refused"] > 0 and k["lit"] > 0 and k["lane_mismatches"] == 0      # see the module docstring
    c, scb, depth, normal, randvec, ref = frame(140, 24, sky, cull, "allsky")
    k = spl.classify(c.ssao_cb, normal, depth)
    assert k["lit"] == 0 and (k["taken"] == 2 * 12 if sky else k["refused"] == 2 * 12) and k["fallback"] == 0


def test_wide_reach_frames_run_the_fallback(built_lib):
    c, scb, depth, normal, randvec, ref = frame(512, 416, True, True, "wide-allsky")
    k = spl.classify(c.ssao_cb, normal, depth)
    assert k["max_cells"] == 65 and k["over_64"] > 0 and k["taken"] == 4 * 208 and k["lit"] == 0
    c, scb, depth, normal, randvec, ref = frame(512, 416, True, True, "wide-patch")
    k = spl.classify(c.ssao_cb, normal, depth)
    assert k["over_64"] > 0 and k["refused"] > 0 and k["lit"] > 0 and k["taken"] == 0


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(built_lib):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from crychic_renderer_amd import Context
    c = Context(0)
    assert "gfx950" in c.device_name, c.device_name
    yield c
    c.close()


class Device:
    def __init__(self, ctx, built_lib, W, H, c, depth, normal, randvec):
        import torch
        self.torch, self.ctx, self.lib, self.check, self.W, self.H, self.cb = torch, ctx, built_lib.lib, built_lib.check, W, H, c.ssao_cb
        dev = ctx.device
        self.d = torch.from_numpy(depth.view(np.int32)).to(dev)
        self.n = torch.from_numpy(normal).to(dev)
        self.r = torch.from_numpy(randvec).to(dev)
        self.a0 = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=dev)
        self.a1 = torch.zeros_like(self.a0)
        self.edge_bytes = int(self.lib.crychic_edge_plane_bytes(W, H))
        self.edge = torch.zeros((self.edge_bytes,), dtype=torch.uint8, device=dev)

    def ptr(self, t):
        return C.c_void_p(t.data_ptr())

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.ctx.device).cuda_stream)

    def ssao(self, row0, rows):
        self.a0.fill_(0x5A5A)
        self.check(self.lib.crychic_ssao(self.ctx.handle, C.byref(self.cb), self.ptr(self.n), self.ptr(self.d), self.ptr(self.r), self.ptr(self.a0),
                                         self.ptr(self.edge), self.W, self.H, row0, rows, self.stream()))
        self.torch.cuda.synchronize()
        return self.a0.cpu().numpy().view(np.uint16)

    def blur(self, src, dst, horz, row0, rows):
        self.check(self.lib.crychic_ssao_blur(self.ctx.handle, C.byref(self.cb), self.ptr(self.edge), self.ptr(src), self.ptr(dst), self.W, self.H,
                                              horz, row0, rows, self.stream()))
        self.torch.cuda.synchronize()
        return dst.cpu().numpy().view(np.uint16)


def run_frame(ctx, built_lib, oracle, hostsim, W, H, c, scb, depth, normal, randvec, ref, strips):
    dv = Device(ctx, built_lib, W, H, c, depth, normal, randvec)
    h2, w2 = H // 2, W // 2
    # whole frame: the ambient plane, then one blur iteration over the workspace the pass left
    got = dv.ssao(0, h2)
    assert np.array_equal(got, ref), "ambient differs in %d of %d pixels" % ((got != ref).sum(), ref.size)
    ref_h = oracle.blur(scb, normal, depth, ref, True)
    got_h = dv.blur(dv.a0, dv.a1, 1, 0, h2)
    assert np.array_equal(got_h, ref_h), "horizontal sweep differs in %d pixels" % (got_h != ref_h).sum()
    got_v = dv.blur(dv.a1, dv.a0, 0, 0, h2)
    assert np.array_equal(got_v, oracle.blur(scb, normal, depth, ref_h, False))
    # strips with row0 > 0, each over a workspace of its own filled with garbage: the strip's ambient rows, what the prologue
    # stores into the workspace (against the host build of the same bodies), and the horizontal sweep over the strip
    n = w2 * h2
    for row0, rows in strips:
        dv.edge.fill_(0xC3)
        got = dv.ssao(row0, rows)
        assert np.array_equal(got[row0:row0 + rows], ref[row0:row0 + rows]), (row0, rows)
        _, hedge = hostsim.ssao(scb, normal, depth, randvec, dv.edge_bytes, row0=row0, rows=rows)
        dedge = dv.edge.cpu().numpy()
        for name, lo, hi in (("nrm", 8 * row0 * w2, 8 * (row0 + rows) * w2), ("vz", 8 * n + 4 * row0 * w2, 8 * n + 4 * (row0 + rows) * w2),
                             ("gcol", 16 * n + 8 * row0, 16 * n + 8 * (row0 + rows)), ("grow", 16 * n + 8 * h2, 16 * n + 8 * h2 + 8 * w2)):
            assert np.array_equal(dedge[lo:hi], hedge[lo:hi]), (name, row0, rows)
        grow = dedge[16 * n + 8 * h2:16 * n + 8 * h2 + 8 * w2].view(np.uint16).reshape(w2, 4)
        assert np.array_equal(grow, normal.view(np.uint16)[0, 1::2]), "grow is not texel row 0"
        got_h = dv.blur(dv.a0, dv.a1, 1, row0, rows)
        assert np.array_equal(got_h[row0:row0 + rows], oracle.blur(scb, normal, depth, ref, True, row0, rows)[row0:row0 + rows]), (row0, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("sky,cull", SWITCHES)
def test_prologue_bit_exact(ctx, built_lib, oracle, hostsim, W, H, sky, cull):
    c, scb, depth, normal, randvec, ref = frame(W, H, sky, cull)
    run_frame(ctx, built_lib, oracle, hostsim, W, H, c, scb, depth, normal, randvec, ref, STRIPS[(W, H)])


@pytest.mark.gpu
@pytest.mark.parametrize("sky", [True, False])
def test_all_sky_short_wavefront(ctx, built_lib, oracle, hostsim, sky):
    """140 x 24, all sky: the 6-lane wavefronts take the shortcut with two cells dealt to six lanes (or, shortcut off, run their taps)."""
    c, scb, depth, normal, randvec, ref = frame(140, 24, sky, True, "allsky")
    assert (ref == 65535).all()
    run_frame(ctx, built_lib, oracle, hostsim, 140, 24, c, scb, depth, normal, randvec, ref, STRIPS[(140, 24)])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["wide-allsky", "wide-patch"])
def test_large_rectangle_fallback(ctx, built_lib, oracle, hostsim, kind):
    """512 x 416, reach over the whole frame: rectangles of 65 cells, served by the fallback loop -- with nothing in them (shortcut
    taken) and with ground along the bottom of the frame (refused)."""
    c, scb, depth, normal, randvec, ref = frame(512, 416, True, True, kind)
    run_frame(ctx, built_lib, oracle, hostsim, 512, 416, c, scb, depth, normal, randvec, ref, ((100, 9),))
