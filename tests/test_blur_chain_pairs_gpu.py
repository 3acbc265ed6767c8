"""blur_replay_chain_kernel with two horizontally adjacent tiles per workgroup and the decision words fetched ahead of the wait
(csrc/kernels.hip), on the frames of tests/blur_masks_lib.py: a lone last tile with a ragged right edge, one tile column, three
tile rows, two full pairs per row; blurCount 2, 3, 4 and 9; strips whose rows cut tiles; sky placed so that the left tile only, the
right tile only, both and neither of a pair are settled; recycled and pre-filled workspaces.  Every map is compared bit for bit
with the oracle AND with the per-iteration plan (CRYCHIC_BLUR_PER_ITERATION=1: one fresh child process renders every case, the
switch is read once per process), and crychic_blur_chain_status reads 0 after every case."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import blur_masks_lib

try:
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

# (frame, blurCount, (row0, rows) or None = the whole map)
CASES = [("322x190", 2, None), ("322x190", 3, None), ("322x190", 4, None), ("322x190", 9, None),
         ("128x64", 3, None), ("128x64", 9, None), ("260x70", 2, None), ("260x70", 4, None), ("512x416", 4, None),
         ("sky", 2, None), ("sky", 3, None), ("sky", 4, None), ("sky", 9, None),
         # (37, 20), blurCount 4: the replayed iterations owe rows 27 .. 66, 32 .. 61, 37 .. 56 -- tile rows 1 and 4 are in the launch
         # and own no row of the last iteration
         ("322x190", 4, (37, 20)), ("512x416", 4, (37, 20)), ("260x70", 3, (17, 5)), ("sky", 4, (100, 61)), ("322x190", 9, (0, 7))]


def case_id(case):
    name, blur_count, strip = case
    return "%s-b%d" % (name, blur_count) + ("-rows%d+%d" % strip if strip else "")


@pytest.fixture(scope="module")
def ctx(built_lib):
    if torch is None or not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from crychic_renderer_amd import Context
    c = Context(0)
    assert "gfx950" in c.device_name, c.device_name
    yield c
    c.close()


def ptr(t):
    return C.c_void_p(t.data_ptr())


class Frame:
    def __init__(self, ctx, lib, name):
        self.W, self.H, self.c, self.scb, self.depth, self.normal, self.randvec = blur_masks_lib.frame(name)
        dev = ctx.device
        self.d = torch.from_numpy(self.depth.view(np.int32)).to(dev)
        self.n = torch.from_numpy(self.normal).to(dev)
        self.r = torch.from_numpy(self.randvec).to(dev)
        self.a0 = torch.zeros((self.H // 2, self.W // 2), dtype=torch.int16, device=dev)
        self.a1 = torch.zeros_like(self.a0)
        self.edge = torch.zeros((int(lib.crychic_edge_plane_bytes(self.W, self.H)),), dtype=torch.uint8, device=dev)
        self.want = {}

    def oracle_map(self, oracle, blur_count):
        if blur_count not in self.want:
            self.want[blur_count] = oracle.compute_ssao(self.scb, self.normal, self.depth, self.randvec, blur_count)
        return self.want[blur_count]

    def run(self, ctx, lib, check, blur_count, strip, edge=None):
        """One crychic_ssao_compute over poisoned planes -> (the strip's rows of ambient0, chain status)."""
        row0, rows = strip or (0, self.H // 2)
        s = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
        self.a0.fill_(0x1111); self.a1.fill_(0x2222)
        check(lib.crychic_ssao_compute(ctx.handle, C.byref(self.c.ssao_cb), ptr(self.n), ptr(self.d), ptr(self.r), ptr(self.a0), ptr(self.a1),
                                       ptr(self.edge if edge is None else edge), self.W, self.H, blur_count, row0, rows, s))
        torch.cuda.synchronize()
        flag = C.c_uint32(7)
        check(lib.crychic_blur_chain_status(ctx.handle, s, C.byref(flag)))
        return self.a0[row0:row0 + rows].cpu().numpy().view(np.uint16), flag.value


_frames = {}


def get_frame(ctx, lib, name):
    if name not in _frames:
        _frames[name] = Frame(ctx, lib, name)
    return _frames[name]


CHILD = """
import sys, ctypes as C, numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import blur_masks_lib
from crychic_renderer_amd import Context
from crychic_renderer_amd._lib import lib, check
ctx = Context(0)
p = lambda t: C.c_void_p(t.data_ptr())
frames, out = {}, {}
for k, (name, blur_count, strip) in enumerate(%(cases)r):
    if name not in frames:
        W, H, c, scb, depth, normal, randvec = blur_masks_lib.frame(name)
        frames[name] = (W, H, c, torch.from_numpy(depth.view(np.int32)).to(ctx.device), torch.from_numpy(normal).to(ctx.device),
                        torch.from_numpy(randvec).to(ctx.device), torch.zeros((int(lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=ctx.device))
    W, H, c, d, n, r, e = frames[name]
    row0, rows = strip or (0, H // 2)
    a0 = torch.full((H // 2, W // 2), 0x1111, dtype=torch.int16, device=ctx.device); a1 = torch.full_like(a0, 0x2222)
    s = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.ssao_cb), p(n), p(d), p(r), p(a0), p(a1), p(e), W, H, blur_count, row0, rows, s))
    torch.cuda.synchronize()
    out['case%%d' %% k] = a0[row0:row0 + rows].cpu().numpy().view(np.uint16)
np.savez(%(out)r, **out)
print('ok')
"""


@pytest.fixture(scope="module")
def per_iteration(ctx):
    """case index -> the strip's rows of the map one launch per iteration gives (a child process with CRYCHIC_BLUR_PER_ITERATION=1)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "maps.npz")
        code = CHILD % dict(root=root, tests=os.path.join(root, "tests"), cases=CASES, out=out)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CRYCHIC_BLUR_PER_ITERATION="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
        with np.load(out) as z:
            return {k: z["case%d" % k] for k in range(len(CASES))}


@pytest.mark.parametrize("k", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_pairs_equal_oracle_and_per_iteration_plan(ctx, built_lib, oracle, per_iteration, k):
    name, blur_count, strip = CASES[k]
    lib, check = built_lib.lib, built_lib.check
    f = get_frame(ctx, lib, name)
    row0, rows = strip or (0, f.H // 2)
    want = f.oracle_map(oracle, blur_count)[row0:row0 + rows]
    got, status = f.run(ctx, lib, check, blur_count, strip)
    assert status == 0
    assert np.array_equal(per_iteration[k], want), "per-iteration plan differs from the oracle in %d texels" % int((per_iteration[k] != want).sum())
    assert np.array_equal(got, want), "%d texels differ from the oracle" % int((got != want).sum())
    assert np.array_equal(got, per_iteration[k])


def test_every_kind_of_pair_occurs(ctx, built_lib, hostsim):
    """The sky frame at blurCount 2, counted with the host build of the pair launch's settle predicate: pairs with the left tile
    only settled, the right tile only, both, and neither all occur; on the other frames no tile settles."""
    bm = blur_masks_lib.load()
    for name in blur_masks_lib.FRAMES:
        W, H, c, scb, depth, normal, randvec = blur_masks_lib.frame(name)
        eb = int(built_lib.lib.crychic_edge_plane_bytes(W, H))
        _, settled = bm.compute_ssao(hostsim, c.ssao_cb, normal, depth, randvec, eb, 2, body=1)
        kinds = blur_masks_lib.pair_cases(settled)
        print(name, "pairs (left only, right only, both, neither settled):", kinds)
        if name == "sky":
            assert all(n >= 1 for n in kinds), kinds
        else:
            assert settled.sum() == 0


def test_recycled_and_prefilled_workspace(ctx, built_lib, oracle):
    """The plain 512 x 416 wall over the workspace the sky frame left (same size, nothing cleared: other tiles were settled, other
    counters published), then over one whose every 32-bit word is the stamp the call will draw, then over one whose every 64-bit
    word reads "this frame, three iterations done" to the chain's poll."""
    lib, check = built_lib.lib, built_lib.check
    sky, wall = get_frame(ctx, lib, "sky"), get_frame(ctx, lib, "512x416")
    want = wall.oracle_map(oracle, 4)
    got, status = sky.run(ctx, lib, check, 4, None)
    assert status == 0 and np.array_equal(got, sky.oracle_map(oracle, 4))
    got, status = wall.run(ctx, lib, check, 4, None, edge=sky.edge)
    assert status == 0 and np.array_equal(got, want)
    words = sky.edge.view(torch.int32).cpu().numpy().view(np.uint32)
    stamps = words[(words >= 0x5EED0000) & (words < 0x5EEE0000)]
    assert stamps.size > 0
    nxt = int(stamps.max()) + 1
    sky.edge.view(torch.int32).fill_(int(np.uint32(nxt).view(np.int32)))
    got, status = wall.run(ctx, lib, check, 4, None, edge=sky.edge)
    assert status == 0 and np.array_equal(got, want)
    assert (sky.edge.view(torch.int32).cpu().numpy().view(np.uint32) == nxt).any(), "the pre-filled value was not the stamp the call drew"
    n64 = sky.edge.numel() // 8
    sky.edge[:n64 * 8].view(torch.int64).fill_(((nxt + 1) << 8) | 3)
    got, status = wall.run(ctx, lib, check, 4, None, edge=sky.edge)
    assert status == 0 and np.array_equal(got, want)
    assert (sky.edge.view(torch.int32).cpu().numpy().view(np.uint32) == nxt + 1).any(), "the pre-filled tag was not the stamp the call drew"
