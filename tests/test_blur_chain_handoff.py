"""The blur chain's tile hand-off under the conditions the other chain tests avoid (kernels.hip blur_replay_chain_kernel: a tile's
workgroup stores its texels and publishes a counter, its neighbours poll the counter and read the texels as their apron).

Input: fuzz_util.rough_wall_case -- no tile settles, every texel changes under the blur, so every tile takes part in the
hand-off and one stale apron texel changes the result; with sky blocks a share of the workgroups returns at once (uneven load).
CPU twin: the kernel bodies on the host against the oracle on these frames, with conditions on the input so that the probe
cannot quietly stop biting.  GPU: a fixed run of 100 frames per configuration on one stream without host synchronisation,
every word of every frame compared on the device with a map made by separate sweep launches (kernel boundaries, none of the
pair / replay / chain kernels) -- idle, next to a stream of large copies, and as row strips.  A parity run of fixed length,
not a hunt: a frame that differs is a finding to be explained from the assembly (tools/handoff_isa.py), not to be re-run."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fuzz_util

FRAMES = 100
BLUR_COUNTS = (2, 3, 4, 8)
SEED = {False: 5, True: 1}


def tiles_of(W, H):
    return ((W // 2 + 63) // 64) * ((H // 2 + 15) // 16)


# ---- CPU twin -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sky_blocks", [False, True])
@pytest.mark.parametrize("W,H", [(770, 400), (1024, 576)])
def test_rough_wall_on_the_host(built_lib, oracle, hostsim, W, H, sky_blocks):
    """hostsim.compute_ssao == oracle.compute_ssao on the rough wall, blurCount 2, 4, 8; without sky blocks no tile settles, with
    them (blurCount 2) between 5 % and 50 % of the tiles do."""
    c, scb, depth, normal, randvec = fuzz_util.rough_wall_case(SEED[sky_blocks], W, H, sky_blocks)
    eb = int(built_lib.lib.crychic_edge_plane_bytes(W, H))
    raw = oracle.ssao(scb, normal, depth, randvec)
    for blur_count in (2, 4, 8):
        want = oracle.compute_ssao(scb, normal, depth, randvec, blur_count)
        got, _ = hostsim.compute_ssao(c.ssao_cb, normal, depth, randvec, eb, blur_count)
        settled = int(hostsim.lib.hs_last_settled_tiles())
        assert np.array_equal(got, want), (blur_count, int((got != want).sum()))
        if not sky_blocks:
            assert settled == 0, (blur_count, settled)
            assert (want != raw).mean() > 0.95 and (raw < 65535).mean() > 0.8      # the blur changes what it touches; the wall occludes
        elif blur_count == 2:
            assert 0.05 * tiles_of(W, H) <= settled <= 0.50 * tiles_of(W, H), (settled, tiles_of(W, H))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

try:
    import torch
except ImportError:         # the CPU twin above needs none
    torch = None


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


def stream(ctx):
    return C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)


class Wall:
    """One rough-wall frame on the host and on the device, with its planes and workspace."""

    def __init__(self, ctx, lib, W, H, sky_blocks):
        self.W, self.H = W, H
        self.c, self.scb, self.depth, self.normal, self.randvec = fuzz_util.rough_wall_case(SEED[sky_blocks], W, H, sky_blocks)
        dev = ctx.device
        self.d = torch.from_numpy(self.depth.view(np.int32)).to(dev)
        self.n = torch.from_numpy(self.normal).to(dev)
        self.r = torch.from_numpy(self.randvec).to(dev)
        self.a0 = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=dev)
        self.a1 = torch.zeros_like(self.a0)
        self.edge = torch.zeros((int(lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=dev)
        self.want = {}

    def expected(self, ctx, lib, check, oracle, blur_count):
        """crychic_ssao + 2 x blurCount separate sweep launches; compared with the oracle where the host can afford it."""
        if blur_count not in self.want:
            W, H = self.W, self.H
            e0, e1 = torch.zeros_like(self.a0), torch.zeros_like(self.a0)
            check(lib.crychic_ssao(ctx.handle, C.byref(self.c.ssao_cb), ptr(self.n), ptr(self.d), ptr(self.r), ptr(e0), ptr(self.edge), W, H, 0, H // 2, stream(ctx)))
            for _ in range(blur_count):
                check(lib.crychic_ssao_blur(ctx.handle, C.byref(self.c.ssao_cb), ptr(self.edge), ptr(e0), ptr(e1), W, H, 1, 0, H // 2, stream(ctx)))
                check(lib.crychic_ssao_blur(ctx.handle, C.byref(self.c.ssao_cb), ptr(self.edge), ptr(e1), ptr(e0), W, H, 0, 0, H // 2, stream(ctx)))
            torch.cuda.synchronize()
            if W * H <= 1024 * 1024 or (os.cpu_count() or 1) >= 32:
                ref = oracle.compute_ssao(self.scb, self.normal, self.depth, self.randvec, blur_count)
                got = e0.cpu().numpy().view(np.uint16)
                print("%dx%d blurCount %d: sweep-by-sweep map against the oracle, %d texels differ" % (W, H, blur_count, int((got != ref).sum())))
                assert np.array_equal(got, ref), "sweep-by-sweep map differs from the oracle in %d texels" % int((got != ref).sum())
            self.want[blur_count] = e0
        return self.want[blur_count]


_walls = {}


def get_wall(ctx, lib, W, H, sky_blocks):
    key = (W, H, sky_blocks)
    if key not in _walls:
        _walls.clear()          # one 4K frame with its maps at a time
        _walls[key] = Wall(ctx, lib, W, H, sky_blocks)
    return _walls[key]


def run_frames(ctx, lib, check, w, want, blur_count, bad, strips=1, frames=FRAMES):
    """frames x (poison both planes, crychic_ssao_compute, count the texels that differ from `want` into the device scalar `bad`);
    no host synchronisation.  strips > 1: every frame as that many row strips, the strip's rows compared after its call."""
    W, H = w.W, w.H
    for _ in range(frames):
        for rank in range(strips):
            r0, rn = C.c_uint32(0), C.c_uint32(H)
            if strips > 1:
                check(lib.crychic_strip_rows(H, strips, rank, C.byref(r0), C.byref(rn)))
            row0, rows = r0.value // 2, rn.value // 2
            w.a0.fill_(0x1111); w.a1.fill_(0x2222)
            check(lib.crychic_ssao_compute(ctx.handle, C.byref(w.c.ssao_cb), ptr(w.n), ptr(w.d), ptr(w.r), ptr(w.a0), ptr(w.a1), ptr(w.edge),
                                           W, H, blur_count, row0, rows, stream(ctx)))
            bad += (w.a0[row0:row0 + rows] != want[row0:row0 + rows]).sum()


def finish(ctx, lib, check, bad, what):
    torch.cuda.synchronize()
    flag = C.c_uint32(7)
    check(lib.crychic_blur_chain_status(ctx.handle, stream(ctx), C.byref(flag)))
    print("%s: %d texels differ over %d frames, chain status %d" % (what, int(bad.item()), FRAMES, flag.value))
    assert int(bad.item()) == 0, "%s: %d texels differ over %d frames" % (what, int(bad.item()), FRAMES)
    assert flag.value == 0, what


def timed(fn):
    """Milliseconds of fn() on the current stream (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


@pytest.mark.gpu
@pytest.mark.parametrize("blur_count", BLUR_COUNTS)
@pytest.mark.parametrize("sky_blocks", [False, True])
@pytest.mark.parametrize("W,H", [(770, 400), (3840, 2160)])
def test_chain_handoff_every_word_of_100_frames(ctx, built_lib, oracle, W, H, blur_count, sky_blocks):
    """3840 x 2160: 30 x 68 tiles, several rounds of workgroups per layer; 770 x 400: a ragged tile grid whose rows are not 128-byte
    aligned.  Idle, then with a second stream kept busy by device-to-device copies of a 1 GiB buffer (as many as cover the run, from
    a timing of one copy and one frame), then -- at 4K -- every frame as eight row strips."""
    lib, check = built_lib.lib, built_lib.check
    w = get_wall(ctx, lib, W, H, sky_blocks)
    want = w.expected(ctx, lib, check, oracle, blur_count)
    dev = ctx.device
    what = "%dx%d blurCount %d %s" % (W, H, blur_count, "sky blocks" if sky_blocks else "plain")

    bad = torch.zeros((), dtype=torch.int64, device=dev)
    run_frames(ctx, lib, check, w, want, blur_count, bad)
    finish(ctx, lib, check, bad, what + ", idle")

    # uneven load from outside the kernel
    src = torch.empty((1 << 30,), dtype=torch.uint8, device=dev).fill_(0x3C)
    dst = torch.empty_like(src)
    side = torch.cuda.Stream(dev)
    one = torch.zeros((), dtype=torch.int64, device=dev)
    run_frames(ctx, lib, check, w, want, blur_count, one, frames=1)      # warm, then timed
    t_frame = timed(lambda: run_frames(ctx, lib, check, w, want, blur_count, one, frames=1))
    dst.copy_(src)
    t_copy = timed(lambda: dst.copy_(src))
    copies = int(math.ceil(FRAMES * t_frame / max(t_copy, 1e-3))) + 2
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(copies):
            dst.copy_(src)
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    run_frames(ctx, lib, check, w, want, blur_count, bad)
    finish(ctx, lib, check, bad, what + ", beside %d copies of 1 GiB (%.3f ms each, a frame %.3f ms)" % (copies, t_copy, t_frame))
    side.synchronize()
    assert int(one.item()) == 0
    del src, dst

    if (W, H) == (3840, 2160):
        bad = torch.zeros((), dtype=torch.int64, device=dev)
        run_frames(ctx, lib, check, w, want, blur_count, bad, strips=8)
        finish(ctx, lib, check, bad, what + ", eight row strips")


CHILD = """
import sys, ctypes as C, numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import fuzz_util
from crychic_renderer_amd import Context
from crychic_renderer_amd._lib import lib, check
ctx = Context(0); W, H = 770, 400
p = lambda t: C.c_void_p(t.data_ptr())
for sky in (False, True):
    c, scb, depth, normal, randvec = fuzz_util.rough_wall_case(%(seed)r[sky], W, H, sky)
    d = torch.from_numpy(depth.view(np.int32)).to(ctx.device); n = torch.from_numpy(normal).to(ctx.device); r = torch.from_numpy(randvec).to(ctx.device)
    a0 = torch.full((H // 2, W // 2), 0x1111, dtype=torch.int16, device=ctx.device); a1 = torch.full_like(a0, 0x2222)
    e = torch.zeros((int(lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=ctx.device)
    s = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.ssao_cb), p(n), p(d), p(r), p(a0), p(a1), p(e), W, H, 4, 0, H // 2, s))
    torch.cuda.synchronize()
    assert np.array_equal(a0.cpu().numpy().view(np.uint16), np.load(%(want)r %% int(sky))), 'per-iteration plan differs (sky blocks %%s)' %% sky
print('ok')
"""


@pytest.mark.gpu
def test_per_iteration_plan_gives_the_same_bytes(ctx, built_lib, oracle):
    """One frame of each 770 x 400 wall through one launch per iteration (CRYCHIC_BLUR_PER_ITERATION=1; the switch is read once per
    process, so a fresh child process) equals the sweep-by-sweep map."""
    lib, check = built_lib.lib, built_lib.check
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        for sky in (False, True):
            want = get_wall(ctx, lib, 770, 400, sky).expected(ctx, lib, check, oracle, 4)
            np.save(os.path.join(d, "want%d.npy" % int(sky)), want.cpu().numpy().view(np.uint16))
        code = CHILD % dict(root=root, tests=os.path.join(root, "tests"), seed=SEED, want=os.path.join(d, "want%d.npy"))
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CRYCHIC_BLUR_PER_ITERATION="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
