"""The dispatch order of the SSAO and lighting launches on the device (csrc/dispatch_order.hpp).  A wrong permutation shows as a band
that nobody wrote or that two workgroup rows own, so the output planes are filled with a poison value, the pass runs, and every
plane is compared with the oracle bit for bit.  The frame is 130 pixels wide (three tile columns, the last ragged); the heights
give every band count around the thresholds of the map -- 1, ways - 1, ways, ways + 1, 2 ways - 1, 2 ways, 2 ways + 1 for the
`ways` the library is built with (read from the header through the host shim of tests/test_dispatch_order.py) -- with whole and
ragged last bands, and one strip inside the frame per pass."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import scene_util
from local_lights_util import as_or_lights
from test_dispatch_order import build_shim

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W = 130
POISON8, POISON16 = 0x5A, 0x5A5A


def band_counts(ways):
    w = max(int(ways), 2)          # natural order and reversal have no thresholds: the counts of two segments
    return sorted({n for n in (1, w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1) if n >= 1})


def ssao_heights(ways):
    """An SSAO band is one row of super-tiles, 128 pixel rows: ceil(H / 128) bands.  Whole and ragged last bands alternate."""
    return [128 * n - (0 if i % 2 else 36) for i, n in enumerate(band_counts(ways))]


def light_heights(ways):
    """A lighting band is 8 tile rows, 32 pixel rows; the rows past the last whole band stay in place: (ceil(H / 4)) // 8 bands.
    32 n: whole bands; 32 n + 10: no multiple of 4; 32 n + 12: a multiple of 4, not of 32."""
    return [32 * n + (0, 10, 12)[i % 3] for i, n in enumerate(band_counts(ways))]


def test_the_heights_hit_the_band_counts():
    for ways in (0, 1, 2, 3, 4):
        assert [-(-h // 128) for h in ssao_heights(ways)] == band_counts(ways)
        hs = light_heights(ways)
        assert [-(-h // 4) // 8 for h in hs] == band_counts(ways)
        assert any(h % 32 and not h % 4 for h in hs) and any(h % 4 for h in hs) and all(h % 2 == 0 for h in hs)


@pytest.fixture(scope="module")
def ctx(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ways():
    s = build_shim()
    return s.shim_ssao_ways(), s.shim_light_ways()


class Frame:
    """One seeded 130 x H scene, its device copies and the oracle's SSAO map (the lighting pass's ambient input)."""

    def __init__(self, ctx, oracle, H):
        pl = scene_util.cpu_scene(W, H, 256, 32)
        self.H, self.c = H, pl["consts"]
        self.p = scene_util.np_planes(pl)
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).to(ctx.device)
                    for k, v in self.p.items()}
        self.scb = oracle_lib.as_oracle_cb(self.c.ssao_cb, oracle_lib.OrSsaoConstants)
        self.pcb = oracle_lib.as_oracle_cb(self.c.pass_cb, oracle_lib.OrPassConstants)
        self.ao = oracle.ssao(self.scb, self.p["normal"], self.p["depth"], self.p["randvec"])
        self.shadow_ptrs = (C.c_void_p * 4)(*[self.dev["shadow"][k].data_ptr() for k in range(4)])


_frames = {}


def frame(ctx, oracle, H):
    if H not in _frames:
        _frames[H] = Frame(ctx, oracle, H)
    return _frames[H]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(ctx):
    return C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)


def run_ssao(ctx, built_lib, f, row0, rows):
    lib, check = built_lib.lib, built_lib.check
    amb = torch.full((f.H // 2, W // 2), POISON16, dtype=torch.int16, device=ctx.device)
    edge = torch.zeros((int(lib.crychic_edge_plane_bytes(W, f.H)),), dtype=torch.uint8, device=ctx.device)
    check(lib.crychic_ssao(ctx.handle, C.byref(f.c.ssao_cb), ptr(f.dev["normal"]), ptr(f.dev["depth"]), ptr(f.dev["randvec"]), ptr(amb),
                           ptr(edge), W, f.H, row0, rows, stream(ctx)))
    torch.cuda.synchronize()
    return amb.cpu().numpy().view(np.uint16)


def run_light(ctx, built_lib, f, row0, rows, points=None):
    lib, check = built_lib.lib, built_lib.check
    out = torch.full((f.H, W, 4), POISON8, dtype=torch.uint8, device=ctx.device)
    rad = torch.full((f.H, W, 4), float("nan"), dtype=torch.float32, device=ctx.device)
    amb = torch.from_numpy(f.ao.view(np.int16)).to(ctx.device)
    args = [ctx.handle, C.byref(f.c.pass_cb), ptr(f.dev["g0"]), ptr(f.dev["g1"]), ptr(f.dev["g2"]), ptr(f.dev["depth"]), ptr(amb),
            f.shadow_ptrs, f.p["shadow"].shape[1], ptr(f.dev["cube"]), f.p["cube"].shape[1], ptr(out), ptr(rad), W, f.H, row0, rows, 3, 0.0, 1]
    if points is None:
        check(lib.crychic_deferred_light(*args, stream(ctx)))
    else:
        host = torch.from_numpy(np.frombuffer(bytes(points), dtype=np.uint8).copy()).to(ctx.device)
        check(lib.crychic_deferred_light_points(*args, ptr(host), len(points), stream(ctx)))
    torch.cuda.synchronize()
    return out.cpu().numpy(), rad.cpu().numpy().view(np.uint32)


def light_ref(oracle, f, row0=0, rows=None, points=None):
    return oracle.deferred_light(f.pcb, f.p["g0"], f.p["g1"], f.p["g2"], f.p["depth"], f.ao, f.p["shadow"], f.p["cube"], 3, 0.0, sky=True,
                                 want_radiance=True, row0=row0, rows=rows, point_lights=None if points is None else as_or_lights(points))


def test_ssao_writes_every_band_once(ctx, built_lib, oracle, ways):
    for H in ssao_heights(ways[0]) + [700]:
        f = frame(ctx, oracle, H)
        got = run_ssao(ctx, built_lib, f, 0, H // 2)
        assert np.array_equal(got, f.ao), (H, "ambient differs in %d of %d pixels" % ((got != f.ao).sum(), f.ao.size))
    assert f.ao.min() < 65535 and (f.ao == 65535).any()


def test_ssao_strip_inside_the_frame(ctx, built_lib, oracle, ways):
    H = 700
    f = frame(ctx, oracle, H)
    row0, rows = 12, 300                                        # half-res rows: 75 tile rows, five bands of the strip's own grid
    got = run_ssao(ctx, built_lib, f, row0, rows)
    assert np.array_equal(got[row0:row0 + rows], f.ao[row0:row0 + rows])
    assert (got[:row0] == POISON16).all() and (got[row0 + rows:] == POISON16).all(), "rows outside the strip were written"


def test_light_writes_every_band_once(ctx, built_lib, oracle, ways):
    for H in light_heights(ways[1]):
        f = frame(ctx, oracle, H)
        ref, ref_rad = light_ref(oracle, f)
        got, got_rad = run_light(ctx, built_lib, f, 0, H)
        assert np.array_equal(got, ref), (H, "RGBA8 differs in %d of %d channels" % ((got != ref).sum(), ref.size))
        assert np.array_equal(got_rad, ref_rad.view(np.uint32)), H


def test_point_light_kernels_follow_the_same_rule(ctx, built_lib, oracle, ways):
    from crychic_renderer_amd import scene
    H = light_heights(ways[1])[-1]                              # 2 ways + 1 bands
    f = frame(ctx, oracle, H)
    L = scene.point_light_grid(4)
    ref, ref_rad = light_ref(oracle, f, points=L)
    got, got_rad = run_light(ctx, built_lib, f, 0, H, points=L)
    assert np.array_equal(got, ref) and np.array_equal(got_rad, ref_rad.view(np.uint32))


def test_light_strip_inside_the_frame(ctx, built_lib, oracle, ways):
    H = 300
    f = frame(ctx, oracle, H)
    row0, rows = 8, 202                                         # 51 tile rows: six bands and three rows past them, the last ragged
    ref, ref_rad = light_ref(oracle, f, row0, rows)
    got, got_rad = run_light(ctx, built_lib, f, row0, rows)
    assert np.array_equal(got[row0:row0 + rows], ref[row0:row0 + rows])
    assert np.array_equal(got_rad[row0:row0 + rows], ref_rad.view(np.uint32)[row0:row0 + rows])
    assert (got[:row0] == POISON8).all() and (got[row0 + rows:] == POISON8).all(), "rows outside the strip were written"
