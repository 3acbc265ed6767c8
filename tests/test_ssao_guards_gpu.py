"""Device tier of the guard sweep (tests/ssao_guard_cases.py; CPU tier: tests/test_ssao_guards_host.py): per case the launchers take
whichever kernel variants the guards pick for its constants -- sky exit on or off with the maps present, tap culling on or off,
clear cells stored or not, the blur chain with and without its exits -- and every result must equal the oracle bit for bit
(uint16 maps, no tolerance): crychic_ssao with the workspace and without one, over two row strips on a workspace of 0xFF bytes,
crychic_ssao_compute at three blur iterations over the whole map and the strips with both planes poisoned before each call, and no
workgroup of a chain may have timed out.  Each case runs twice on one workspace: the second frame may not lean on the first's."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import ssao_guard_cases as G

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from crychic_renderer_amd import Context
    c = Context(0)
    assert "gfx950" in c.device_name, c.device_name
    yield c
    c.close()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev_u16(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_guard_case_on_device(ctx, built_lib, oracle, case):
    f = G.build_frame(case)
    W, H, h2 = f.W, f.H, f.H // 2
    assert W <= 640 and H <= 384
    lib, check, dev = built_lib.lib, built_lib.check, ctx.device
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    scb = oracle_lib.as_oracle_cb(f.cb, oracle_lib.OrSsaoConstants)
    raw = oracle.ssao(scb, f.normal, f.depth, f.randvec)
    want = oracle.compute_ssao(scb, f.normal, f.depth, f.randvec, G.BLUR_COUNT)
    assert int((raw < 65535).sum()) > 50 and int((raw == 65535).sum()) > 50
    d, n, r = (torch.from_numpy(p.copy()).to(dev) for p in (f.depth.view(np.int32), f.normal, f.randvec))      # the table's planes are read-only
    a0 = torch.zeros((h2, W // 2), dtype=torch.int16, device=dev)
    a1 = torch.zeros_like(a0)
    eb = int(lib.crychic_edge_plane_bytes(W, H))
    edge = torch.zeros((eb,), dtype=torch.uint8, device=dev)
    flag = C.c_uint32(7)

    def ssao(workspace, row0, rows):
        a0.fill_(0x5A5A)
        check(lib.crychic_ssao(ctx.handle, C.byref(f.cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(workspace), W, H, row0, rows, stream))
        torch.cuda.synchronize()
        return dev_u16(a0)[row0:row0 + rows]

    def compute(row0, rows):
        a0.fill_(0x5A5A); a1.fill_(0x2525)
        check(lib.crychic_ssao_compute(ctx.handle, C.byref(f.cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(a1), ptr(edge), W, H, G.BLUR_COUNT, row0, rows,
                                       stream))
        check(lib.crychic_blur_chain_status(ctx.handle, stream, C.byref(flag)))
        assert flag.value == 0
        return dev_u16(a0)[row0:row0 + rows]

    for frame in range(2):
        got = ssao(edge, 0, h2)
        assert np.array_equal(got, raw), (frame, int((got != raw).sum()))
        got = ssao(None, 0, h2)
        assert np.array_equal(got, raw), (frame, "no workspace", int((got != raw).sum()))
        garbage = torch.full((eb,), 0xFF, dtype=torch.uint8, device=dev)
        for row0, rows in G.strips(H):
            got = ssao(garbage, row0, rows)
            assert np.array_equal(got, raw[row0:row0 + rows]), (frame, row0, rows, int((got != raw[row0:row0 + rows]).sum()))
        for row0, rows in ((0, h2),) + G.strips(H):
            got = compute(row0, rows)
            assert np.array_equal(got, want[row0:row0 + rows]), (frame, row0, rows, int((got != want[row0:row0 + rows]).sum()))
