"""GPU parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on the same seeded
inputs.  Bar: BIT-EXACT on every plane (R16 ambient, RGBA8 colour, and the fp32 radiance bits) -- the kernels use
the oracle's IEEE-754 evaluation order (DESIGN.md "Numerical contract"), so no tolerance is needed; where a
tolerance would apply (radiance) it is stated as 0 ulp.  Oracle = oracle/ (parity unpinned, see its header)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import scene_util

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


def to_dev(p, ctx):
    return {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).to(ctx.device)
            for k, v in p.items()}


def dev_u16(t):
    return t.cpu().numpy().view(np.uint16)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(ctx):
    return C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)


class Case:
    """One seeded scene: numpy planes for the oracle + device copies for the HIP path."""

    def __init__(self, ctx, built_lib, W, H, shadow_dim=512, cube_dim=64, device="cpu"):
        from crychic_renderer_amd import scene
        self.W, self.H = W, H
        if device == "cpu":
            self.planes = scene_util.cpu_scene(W, H, shadow_dim, cube_dim)
        else:
            self.planes = scene.make_scene(W, H, shadow_dim=shadow_dim, cube_dim=cube_dim, device=device)
        self.np = scene_util.np_planes(self.planes)
        self.dev = to_dev(self.np, ctx)
        self.consts = self.planes["consts"]
        self.scb = oracle_lib.as_oracle_cb(self.consts.ssao_cb, oracle_lib.OrSsaoConstants)
        self.pcb = oracle_lib.as_oracle_cb(self.consts.pass_cb, oracle_lib.OrPassConstants)
        w2, h2 = W // 2, H // 2
        self.a0 = torch.zeros((h2, w2), dtype=torch.int16, device=ctx.device)
        self.a1 = torch.zeros((h2, w2), dtype=torch.int16, device=ctx.device)
        self.edge = torch.zeros((int(built_lib.lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=ctx.device)
        self.out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
        self.rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
        self.shadow_ptrs = (C.c_void_p * 4)(*[self.dev["shadow"][k].data_ptr() for k in range(4)])


_cases = {}


def get_case(ctx, built_lib, W, H, **kw):
    key = (W, H, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = Case(ctx, built_lib, W, H, **kw)
    return _cases[key]


SIZES = [(64, 64), (256, 256), (322, 190), (130, 34)]


@pytest.mark.parametrize("W,H", SIZES)
def test_ssao_bit_exact(ctx, built_lib, oracle, W, H):
    c = get_case(ctx, built_lib, W, H)
    lib, check = built_lib.lib, built_lib.check
    check(lib.crychic_ssao(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]),
                           ptr(c.dev["randvec"]), ptr(c.a0), ptr(c.edge), W, H, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    ref = oracle.ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"])
    got = dev_u16(c.a0)
    assert np.array_equal(got, ref), "ambient differs in %d of %d pixels" % ((got != ref).sum(), ref.size)
    assert ref.min() < 65535  # the scene really occludes something
    # without a workspace the taps gather from the raw D24 plane instead of the decoded depth-pairs plane: same bits
    c.a0.zero_()
    check(lib.crychic_ssao(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]),
                           ptr(c.dev["randvec"]), ptr(c.a0), None, W, H, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    assert np.array_equal(dev_u16(c.a0), ref)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_tap_culling_on_device(ctx, built_lib, oracle, seed):
    """SSAO tap culling on the device (nearest-depth map built by depth_pairs_kernel, per-lane skipped
    gathers, wave-level skipped tap pairs) against the oracle, on the probe frames of
    tests/test_hostsim_parity.py::test_tap_culling_is_exact_and_bites; then the whole ComputeSsao chain on the same workspace."""
    import fuzz_util
    import oracle_lib
    W, H, c, depth, normal, randvec = fuzz_util.cull_probe_case(seed, 384, 224)
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    lib, check = built_lib.lib, built_lib.check
    dev = ctx.device
    d = torch.from_numpy(depth.view(np.int32)).to(dev); n = torch.from_numpy(normal).to(dev); r = torch.from_numpy(randvec).to(dev)
    a0 = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=dev)
    a1 = torch.zeros_like(a0)
    edge = torch.zeros((int(lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=dev)
    ref = oracle.ssao(scb, normal, depth, randvec)
    check(lib.crychic_ssao(ctx.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(edge), W, H, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    got = dev_u16(a0)
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert (ref < 65535).sum() > 50
    check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(a1), ptr(edge), W, H, 3, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    assert np.array_equal(dev_u16(a0), oracle.compute_ssao(scb, normal, depth, randvec, 3))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_clear_cells_on_device(ctx, built_lib, oracle, seed):
    """depth_pairs_kernel does not write the pairs entries that only clear cells of the nearest-depth map can reach, and
    ssao_kernel never reads them (ssao_core.hpp "clear cells").  The probe frames of
    tests/test_hostsim_parity.py::test_clear_cells_are_never_read over a workspace filled with garbage, whole frame and strips,
    then the ComputeSsao chain."""
    import fuzz_util
    W, H, c, scb, depth, normal, randvec = fuzz_util.clear_cell_probe_case(seed)
    lib, check = built_lib.lib, built_lib.check
    dev = ctx.device
    d = torch.from_numpy(depth.view(np.int32)).to(dev); n = torch.from_numpy(normal).to(dev); r = torch.from_numpy(randvec).to(dev)
    a0 = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=dev)
    a1 = torch.zeros_like(a0)
    ref = oracle.ssao(scb, normal, depth, randvec)
    for fill in (0xC0, 0x00, 0xFF):          # as floats: -6.02, 0.0 (the nearest depth there is), NaN
        edge = torch.full((int(lib.crychic_edge_plane_bytes(W, H)),), fill, dtype=torch.uint8, device=dev)
        check(lib.crychic_ssao(ctx.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(edge), W, H, 0, H // 2, stream(ctx)))
        torch.cuda.synchronize()
        got = dev_u16(a0)
        assert np.array_equal(got, ref), (fill, int((got != ref).sum()))
        for row0, rows in ((0, H // 8), (H // 4, H // 8)):
            a0.zero_()
            check(lib.crychic_ssao(ctx.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(edge), W, H, row0, rows, stream(ctx)))
            torch.cuda.synchronize()
            assert np.array_equal(dev_u16(a0)[row0:row0 + rows], ref[row0:row0 + rows]), (fill, row0)
    assert (ref < 65535).sum() > 50
    check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(a1), ptr(edge), W, H, 3, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    assert np.array_equal(dev_u16(a0), oracle.compute_ssao(scb, normal, depth, randvec, 3))


@pytest.mark.parametrize("W,H", SIZES)
def test_blur_sweeps_bit_exact(ctx, built_lib, oracle, W, H):
    c = get_case(ctx, built_lib, W, H)
    lib, check = built_lib.lib, built_lib.check
    rng = np.random.default_rng(1234 + W)
    amb = rng.integers(0, 65536, size=(H // 2, W // 2), dtype=np.uint16)  # noise: exercises every accept/reject mix
    check(lib.crychic_ssao_edges(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]),
                                 ptr(c.edge), W, H, 0, H // 2, stream(ctx)))
    cur = amb
    for horz in (1, 0, 1, 0):
        c.a0.copy_(torch.from_numpy(cur.view(np.int16)))
        check(lib.crychic_ssao_blur(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.edge), ptr(c.a0), ptr(c.a1), W, H, horz,
                                    0, H // 2, stream(ctx)))
        torch.cuda.synchronize()
        ref = oracle.blur(c.scb, c.np["normal"], c.np["depth"], cur, bool(horz))
        got = dev_u16(c.a1)
        assert np.array_equal(got, ref), "sweep horz=%d differs in %d pixels" % (horz, (got != ref).sum())
        cur = ref


@pytest.mark.parametrize("W,H", [(256, 256), (322, 190), (130, 34)])
@pytest.mark.parametrize("blur_count", [0, 1, 2, 3, 4, 5, 6, 8])
def test_compute_ssao_bit_exact(ctx, built_lib, oracle, W, H, blur_count):
    """Ssao::ComputeSsao: SSAO pass + the two-launch blur chain (iteration 0 as one H + V launch, the rest fused and replayed)
    == the oracle's 1 + 2 * blurCount separate passes, whole map and row strips (halo recomputed per stage), both planes
    poisoned before every call."""
    c = get_case(ctx, built_lib, W, H)
    lib, check = built_lib.lib, built_lib.check
    ref = oracle.compute_ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], blur_count)
    h2 = H // 2
    for row0, rows in ((0, h2), (h2 // 3, h2 // 4 + 1), (h2 - 9, 9)):
        c.a0.fill_(0x5A5A); c.a1.fill_(0x2525)
        check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]),
                                       ptr(c.dev["randvec"]), ptr(c.a0), ptr(c.a1), ptr(c.edge), W, H, blur_count, row0, rows,
                                       stream(ctx)))
        torch.cuda.synchronize()
        got = dev_u16(c.a0)
        assert np.array_equal(got[row0:row0 + rows], ref[row0:row0 + rows]), (row0, rows, int((got[row0:row0 + rows] != ref[row0:row0 + rows]).sum()))


@pytest.mark.parametrize("W,H", [(322, 190), (130, 34)])
@pytest.mark.parametrize("blur_count", [9, 10, 12])
def test_compute_ssao_at_the_chain_plan_boundary(ctx, built_lib, oracle, W, H, blur_count):
    """blurCount 9 is the longest chain that runs as one launch (its 8 replay iterations fill BlurChainPlan); from 10 on api.cpp
    issues one replay launch per iteration in the same process (blurCount - 1 > 8).  Both equal the oracle's sweeps, whole map and
    row strips, both planes poisoned before every call.  crychic_blur_chain_status reports 0 either way: at 9 no workgroup timed
    out; at 10 and 12 no chain ran, and the call answers for the last chain of this context (or 0 if there was none)."""
    c = get_case(ctx, built_lib, W, H)
    lib, check = built_lib.lib, built_lib.check
    ref = oracle.compute_ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], blur_count)
    h2 = H // 2
    flag = C.c_uint32(7)
    for row0, rows in ((0, h2), (h2 // 3, h2 // 4 + 1), (h2 - 9, 9)):
        c.a0.fill_(0x5A5A); c.a1.fill_(0x2525)
        check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]),
                                       ptr(c.dev["randvec"]), ptr(c.a0), ptr(c.a1), ptr(c.edge), W, H, blur_count, row0, rows,
                                       stream(ctx)))
        check(lib.crychic_blur_chain_status(ctx.handle, stream(ctx), C.byref(flag)))
        assert flag.value == 0
        got = dev_u16(c.a0)
        assert np.array_equal(got[row0:row0 + rows], ref[row0:row0 + rows]), (row0, rows, int((got[row0:row0 + rows] != ref[row0:row0 + rows]).sum()))


def test_blur_chain_single_launch_equals_per_iteration(ctx, built_lib, oracle):
    """Iterations 1 .. blurCount - 1 as ONE launch with per-tile dependencies (kernels.hip blur_replay_chain_kernel) against the oracle's
    sweep-by-sweep chain and against one launch per iteration (CRYCHIC_BLUR_PER_ITERATION=1 in a child process): whole maps and
    strips, blurCount 2 .. 8, repeated on one workspace (the counters of the previous frame carry another stamp), and no workgroup
    may have timed out (crychic_blur_chain_status)."""
    import os, subprocess, sys, tempfile
    W, H = 322, 190
    c = get_case(ctx, built_lib, W, H)
    lib, check = built_lib.lib, built_lib.check
    flag = C.c_uint32(7)
    outs = {}
    for blur_count in (2, 3, 4, 8):
        want = oracle.compute_ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], blur_count)
        for rep in range(3):
            c.a0.fill_(0x1111); c.a1.fill_(0x2222)
            check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]), ptr(c.dev["randvec"]),
                                           ptr(c.a0), ptr(c.a1), ptr(c.edge), W, H, blur_count, 0, H // 2, stream(ctx)))
            check(lib.crychic_blur_chain_status(ctx.handle, stream(ctx), C.byref(flag)))
            assert flag.value == 0
            assert np.array_equal(dev_u16(c.a0), want), (blur_count, rep)
        for row0, rows in ((0, 31), (40, 17), (H // 2 - 23, 23)):
            c.a0.fill_(0x1111); c.a1.fill_(0x2222)
            check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]), ptr(c.dev["randvec"]),
                                           ptr(c.a0), ptr(c.a1), ptr(c.edge), W, H, blur_count, row0, rows, stream(ctx)))
            check(lib.crychic_blur_chain_status(ctx.handle, stream(ctx), C.byref(flag)))
            assert flag.value == 0
            assert np.array_equal(dev_u16(c.a0)[row0:row0 + rows], want[row0:row0 + rows]), (blur_count, row0, rows)
        outs[blur_count] = want
    # the per-iteration launch plan in a child process (the switch is read once per process): same bytes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "want.npy"), outs[4])
        code = ("import sys, numpy as np, torch, ctypes as C; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "import scene_util\nfrom crychic_renderer_amd import Context\nfrom crychic_renderer_amd._lib import lib, check\n"
                "ctx = Context(0); W, H = %d, %d\npl = scene_util.cpu_scene(W, H, 512, 64); p = scene_util.np_planes(pl); c = pl['consts']\n"
                "t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(ctx.device)\n"
                "n, d, r = t(p['normal']), t(p['depth']), t(p['randvec'])\n"
                "a0 = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=ctx.device); a1 = torch.zeros_like(a0)\n"
                "e = torch.zeros((int(lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=ctx.device)\n"
                "s = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)\n"
                "check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.ssao_cb), C.c_void_p(n.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(r.data_ptr()),"
                " C.c_void_p(a0.data_ptr()), C.c_void_p(a1.data_ptr()), C.c_void_p(e.data_ptr()), W, H, 4, 0, H // 2, s))\n"
                "torch.cuda.synchronize()\nassert np.array_equal(a0.cpu().numpy().view(np.uint16), np.load(%r)), 'per-iteration plan differs'\nprint('ok')\n"
                % (root, os.path.join(root, "tests"), W, H, os.path.join(d, "want.npy")))
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CRYCHIC_BLUR_PER_ITERATION="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_recycled_workspace_on_device(ctx, built_lib, oracle):
    """The edge workspace is caller-owned and nothing clears it (ADVICE r2 / VERDICT r2 item 2).  Frame A on context 1; context 1
    destroyed; a DIFFERENT frame B on a new context over the same, uncleared workspace; then frame B again over a workspace whose
    every 32-bit word holds the stamp the next call will draw (read back from the map frame A left: stamps come from one
    process-wide counter, one per SSAO pass), and over one whose every 64-bit word is a finished counter of the blur chain for the
    upcoming stamp.  Frame B must equal the oracle each time."""
    import fuzz_util
    from crychic_renderer_amd import Context
    W, H, c, scb, depth_a, normal_a, randvec = fuzz_util.sky_probe_case(0)
    depth_b, normal_b = np.ascontiguousarray(depth_a[::-1, ::-1]), np.ascontiguousarray(normal_a[::-1, ::-1])
    lib, check = built_lib.lib, built_lib.check
    dev = ctx.device
    r = torch.from_numpy(randvec).to(dev)
    a0 = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=dev); a1 = torch.zeros_like(a0)
    edge = torch.zeros((int(lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=dev)
    want_b = oracle.compute_ssao(scb, normal_b, depth_b, randvec, 4)

    def run(context, depth, normal):
        d = torch.from_numpy(depth.view(np.int32)).to(dev); n = torch.from_numpy(normal).to(dev)
        a0.fill_(0x5A5A); a1.fill_(0x2525)
        check(lib.crychic_ssao_compute(context.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(a1), ptr(edge), W, H, 4, 0, H // 2,
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.synchronize()
        return dev_u16(a0).copy()

    c1 = Context(0)
    got_a = run(c1, depth_a, normal_a)
    assert np.array_equal(got_a, oracle.compute_ssao(scb, normal_a, depth_a, randvec, 4))
    c1.close()
    c2 = Context(0)
    try:
        assert np.array_equal(run(c2, depth_b, normal_b), want_b)
        words = edge.view(torch.int32).cpu().numpy().view(np.uint32)
        stamps = words[(words >= 0x5EED0000) & (words < 0x5EEE0000)]
        assert stamps.size > 0
        nxt = int(stamps.max()) + 1
        edge.view(torch.int32).fill_(int(np.uint32(nxt).view(np.int32)))
        assert np.array_equal(run(c2, depth_b, normal_b), want_b)
        words = edge.view(torch.int32).cpu().numpy().view(np.uint32)
        assert (words == nxt).any(), "the pre-filled value was not the stamp the call drew: the probe did not bite"
        # ... and over a workspace whose every 64-bit word reads "this frame, three blur iterations done" to the single-launch chain
        # (its per-tile counters: (stamp << 8) | iterations): the launch before the chain rewrites the counters it will poll
        nxt2 = nxt + 1
        n64 = edge.numel() // 8
        edge[:n64 * 8].view(torch.int64).fill_((nxt2 << 8) | 3)
        assert np.array_equal(run(c2, depth_b, normal_b), want_b)
        flag = C.c_uint32(9)
        check(lib.crychic_blur_chain_status(c2.handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(flag)))
        assert flag.value == 0
        words = edge.view(torch.int32).cpu().numpy().view(np.uint32)
        assert (words == nxt2).any(), "the pre-filled counter tag was not the stamp the call drew: the probe did not bite"
    finally:
        c2.close()


@pytest.mark.parametrize("W,H", [(64, 64), (256, 256), (322, 190)])
@pytest.mark.parametrize("num_dir_lights,literal,sky,ssao_on", [(1, 1, 0, 1), (3, 1, 1, 1), (3, 0, 0, 1), (1, 0, 1, 0)])
def test_deferred_light_bit_exact(ctx, built_lib, oracle, W, H, num_dir_lights, literal, sky, ssao_on):
    c = get_case(ctx, built_lib, W, H)
    lib, check = built_lib.lib, built_lib.check
    amb = oracle.compute_ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], 1) if ssao_on else None
    if ssao_on:
        c.a0.copy_(torch.from_numpy(amb.view(np.int16)))
    radius = lib.crychic_pcf_search_radius(c.np["shadow"].shape[1], literal)
    assert (radius == 0.0) == bool(literal)
    check(lib.crychic_deferred_light(ctx.handle, C.byref(c.consts.pass_cb), ptr(c.dev["g0"]), ptr(c.dev["g1"]),
                                     ptr(c.dev["g2"]), ptr(c.dev["depth"]), ptr(c.a0) if ssao_on else None,
                                     c.shadow_ptrs, c.np["shadow"].shape[1], ptr(c.dev["cube"]), c.np["cube"].shape[1],
                                     ptr(c.out), ptr(c.rad), W, H, 0, H, num_dir_lights, radius, sky, stream(ctx)))
    torch.cuda.synchronize()
    ref, ref_rad = oracle.deferred_light(c.pcb, c.np["g0"], c.np["g1"], c.np["g2"], c.np["depth"], amb, c.np["shadow"],
                                         c.np["cube"], num_dir_lights, radius, sky=bool(sky), want_radiance=True)
    got, got_rad = c.out.cpu().numpy(), c.rad.cpu().numpy()
    assert np.array_equal(got, ref), "RGBA8 differs in %d of %d channels" % ((got != ref).sum(), ref.size)
    # radiance: tolerance 0 ulp (bit pattern equality, NaN-safe)
    assert np.array_equal(got_rad.view(np.uint32), ref_rad.view(np.uint32))


@pytest.mark.parametrize("seed", [0, 1])
def test_dark_light_skip_on_device(ctx, built_lib, oracle, seed):
    """The device twin of tests/test_hostsim_parity.py::test_dark_light_skip_is_exact: a zero-strength directional light is
    skipped, and the other lights take the shorter reciprocals, only on wavefronts whose every pixel is inside the input bounds
    (light_core.hpp "dark lights").  G-buffer values on both sides of every bound, in runs of whole wavefronts and pixel by
    pixel; device == oracle: RGBA8 byte for byte; radiance by bits on every lane that is not NaN, and NaN lanes as NaN == NaN
    (x86 and gfx950 generate NaNs of different sign / payload, 0xFFC00000 against 0x7FC00000; fuzz_util.same_floats).
    The guard bounds the G-buffer, not EyePosW -- the shortcuts stay exact for any eye because every dot product with the view
    vector goes through maxnn(): the last cases run a huge, an infinite and a NaN eye position against the oracle."""
    import copy
    import fuzz_util
    W, H = 256, 64
    c = get_case(ctx, built_lib, 256, 256)
    lib, check = built_lib.lib, built_lib.check
    rng = np.random.default_rng(900 + seed)
    g0, g1, g2 = (c.np[k][:H].copy() for k in ("g0", "g1", "g2"))
    depth = np.full((H, W), 1000, dtype=np.uint32)
    def pick(vals, shape):
        return rng.choice(np.asarray(vals, dtype=np.float32), size=shape)
    # rows 0..31: per-wavefront (64 pixels) constant values, rows 32..63: per pixel
    rough = [0.0, 0.02, 0.03, 0.031, 0.3, 0.8, 1.0, 9.99, 10.0, 10.5, 1e6, np.inf, np.nan, -0.5]
    alb = [0.0, 0.5, 0.9, 1.0, 15.9, 16.0, 16.5, -16.0, -17.0, 1e5, np.nan]
    met = [0.0, 0.5, 1.0, 16.0, 16.01, -16.0, 1e9, np.nan]
    g1[:32, :, 3] = np.repeat(pick(rough, (32, W // 64)), 64, axis=1); g1[32:, :, 3] = pick(rough, (32, W))
    for ch in range(3):
        g1[:32, :, ch] = np.repeat(pick(alb, (32, W // 64)), 64, axis=1); g1[32:, :, ch] = pick(alb, (32, W))
    g0[:32, :, 3] = np.repeat(pick(met, (32, W // 64)), 64, axis=1); g0[32:, :, 3] = pick(met, (32, W))
    bad = rng.random((H, W)) < 0.03
    g0[bad, 0] = pick([np.inf, -np.inf, np.nan, 2e30, 1e30], int(bad.sum()))
    badn = rng.random((H, W)) < 0.03
    g2[badn, 1] = pick([np.inf, np.nan, 0.0, 3.3e38], int(badn.sum()))
    amb = rng.integers(0, 65536, size=(H // 2, W // 2), dtype=np.uint16)
    dev = ctx.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)
    dg0, dg1, dg2, dd, da = t(g0), t(g1), t(g2), t(depth), torch.from_numpy(amb.view(np.int16)).to(dev)
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev); rad = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    cb = copy.deepcopy(c.consts.pass_cb)
    eye0 = tuple(cb.EyePosW)
    for d, strength, eye in (((0.0, -0.707, -0.707), (0.0, 0.0, 0.0), eye0), ((0.0, -1.0004, 0.0), (-0.0, 0.0, -0.0), eye0),
                             ((0.0, -1.01, 0.0), (0.0, 0.0, 0.0), eye0), ((0.0, -0.707, -0.707), (0.0, 1e-30, 0.0), eye0),
                             ((0.0, -0.707, -0.707), (0.0, 0.0, 0.0), (3.0e30, 2.0, -1.0e25)),
                             ((0.0, -0.707, -0.707), (0.0, 0.0, 0.0), (float("inf"), 2.0, -15.0)),
                             ((0.0, -0.707, -0.707), (0.0, 0.0, 0.0), (0.0, float("nan"), -15.0))):
        cb.Lights[2].Direction[:] = d
        cb.Lights[2].Strength[:] = strength
        cb.EyePosW[:] = eye
        ocb = oracle_lib.as_oracle_cb(cb, oracle_lib.OrPassConstants)
        check(lib.crychic_deferred_light(ctx.handle, C.byref(cb), ptr(dg0), ptr(dg1), ptr(dg2), ptr(dd), ptr(da), c.shadow_ptrs, c.np["shadow"].shape[1],
                                         ptr(c.dev["cube"]), c.np["cube"].shape[1], ptr(out), ptr(rad), W, H, 0, H, 3, 0.0, 0, stream(ctx)))
        torch.cuda.synchronize()
        ref, rref = oracle.deferred_light(ocb, g0, g1, g2, depth, amb, c.np["shadow"], c.np["cube"], 3, 0.0, want_radiance=True)
        assert np.array_equal(out.cpu().numpy(), ref), (d, strength, eye)
        assert fuzz_util.same_floats(rad.cpu().numpy(), rref), (d, strength, eye)       # non-NaN lanes by bits, NaN == NaN


@pytest.mark.parametrize("fixes,literal", [(0x100, 1), (0x200, 1), (0x400, 1), (0x700, 0)])
def test_quirk_fix_switches_on_device(ctx, built_lib, oracle, fixes, literal):
    """CRYCHIC_FIX_Q1 / Q3 / Q4 through the C ABI == the oracle with the same switches (RGBA8 and radiance bits)."""
    W, H = 256, 256
    c = get_case(ctx, built_lib, W, H)
    lib, check = built_lib.lib, built_lib.check
    amb = oracle.compute_ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], 1)
    c.a0.copy_(torch.from_numpy(amb.view(np.int16)))
    radius = lib.crychic_pcf_search_radius(c.np["shadow"].shape[1], literal)
    check(lib.crychic_deferred_light(ctx.handle, C.byref(c.consts.pass_cb), ptr(c.dev["g0"]), ptr(c.dev["g1"]),
                                     ptr(c.dev["g2"]), ptr(c.dev["depth"]), ptr(c.a0), c.shadow_ptrs, c.np["shadow"].shape[1],
                                     ptr(c.dev["cube"]), c.np["cube"].shape[1], ptr(c.out), ptr(c.rad), W, H, 0, H, 3, radius, 1 | fixes,
                                     stream(ctx)))
    torch.cuda.synchronize()
    ref, ref_rad = oracle.deferred_light(c.pcb, c.np["g0"], c.np["g1"], c.np["g2"], c.np["depth"], amb, c.np["shadow"], c.np["cube"], 3,
                                         radius, sky=True, want_radiance=True, fixes=fixes)
    assert np.array_equal(c.out.cpu().numpy(), ref)
    assert np.array_equal(c.rad.cpu().numpy().view(np.uint32), ref_rad.view(np.uint32))


def test_draw_hot_path_matches_oracle_and_strips(ctx, built_lib, oracle):
    """crychic_draw_hot_path == oracle ComputeSsao + lighting; rendering the frame as 1, 2, 3 and 8 row strips
    (the multi-GPU decomposition, each strip recomputing its own SSAO/blur halo) gives the same bytes."""
    from crychic_renderer_amd import Crychic
    W, H = 256, 256
    c = get_case(ctx, built_lib, W, H)
    app = Crychic(ctx, W, H, c.dev["randvec"], c.dev["cube"], shadow_dim=c.np["shadow"].shape[1])
    app.load_scene({**c.dev, "consts": c.consts})
    app.blurCount, app.numDirLights = 3, 3
    app.pcfSearchRadius = built_lib.lib.crychic_pcf_search_radius(c.np["shadow"].shape[1], 0)
    app.Draw()
    torch.cuda.synchronize()
    full = app.mBackBuffer.cpu().numpy().copy()
    amb = oracle.compute_ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], 3)
    ref = oracle.deferred_light(c.pcb, c.np["g0"], c.np["g1"], c.np["g2"], c.np["depth"], amb, c.np["shadow"], c.np["cube"],
                                3, app.pcfSearchRadius)
    assert np.array_equal(full, ref)
    for nranks in (2, 3, 8):
        app.mBackBuffer.zero_()
        for rank in range(nranks):
            r0, rn = C.c_uint32(), C.c_uint32()
            built_lib.check(built_lib.lib.crychic_strip_rows(H, nranks, rank, C.byref(r0), C.byref(rn)))
            # poison the AO planes so a strip cannot lean on rows another strip computed
            app.mSsao.mAmbientMap0.fill_(0x5A5A)
            app.mSsao.mAmbientMap1.fill_(0x2525)
            app.Draw(r0.value, rn.value)
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), full), "strip decomposition nranks=%d differs" % nranks


def test_hot_path_replays_from_a_hip_graph(ctx, built_lib, oracle):
    """crychic_draw_hot_path is stream-ordered, allocation-free and never synchronises: a caller can capture it into a hipGraph
    and replay it.  A replay re-uses the frame stamp that was drawn at capture time -- still exact, because every stamped word
    a frame looks at is written earlier in that same frame (crychic_hip.h, workspace contract).  Frame A is captured; then
    different planes are copied into the same buffers and the replay has to give frame B, bit for bit the oracle's."""
    from crychic_renderer_amd import Crychic
    W, H = 256, 256
    c = get_case(ctx, built_lib, W, H)
    planes = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c.dev.items()}
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=c.np["shadow"].shape[1])
    app.load_scene({**planes, "consts": c.consts})
    app.blurCount, app.numDirLights = 3, 3
    app.pcfSearchRadius = built_lib.lib.crychic_pcf_search_radius(c.np["shadow"].shape[1], 0)
    app.Draw()                                   # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        app.Draw()

    def want(normal, depth):
        amb = oracle.compute_ssao(c.scb, normal, depth, c.np["randvec"], 3)
        return oracle.deferred_light(c.pcb, c.np["g0"], c.np["g1"], c.np["g2"], depth, amb, c.np["shadow"], c.np["cube"], 3, app.pcfSearchRadius)

    app.mBackBuffer.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), want(c.np["normal"], c.np["depth"]))
    # frame B: the depth / normal planes upside down (sky where the ground was), in the buffers the graph captured
    depth_b, normal_b = np.ascontiguousarray(c.np["depth"][::-1]), np.ascontiguousarray(c.np["normal"][::-1])
    planes["depth"].copy_(torch.from_numpy(depth_b.view(np.int32)))
    planes["normal"].copy_(torch.from_numpy(normal_b))
    for _ in range(2):
        app.mBackBuffer.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), want(normal_b, depth_b))


def test_c2_1080p_parity(ctx, built_lib, oracle):
    """BASELINE config 2: 1920x1080, 3 lights, 14-sample SSAO + 1 blur pass, vs the oracle."""
    from crychic_renderer_amd import Crychic
    W, H = 1920, 1080
    c = get_case(ctx, built_lib, W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))      # the cascades BASELINE / bench.py use
    app = Crychic(ctx, W, H, c.dev["randvec"], c.dev["cube"], shadow_dim=4096)
    app.load_scene({**c.dev, "consts": c.consts})
    app.blurCount, app.numDirLights = 1, 3
    app.Draw()
    torch.cuda.synchronize()
    amb = oracle.compute_ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], 1)
    assert np.array_equal(dev_u16(app.mSsao.mAmbientMap0), amb)
    ref = oracle.deferred_light(c.pcb, c.np["g0"], c.np["g1"], c.np["g2"], c.np["depth"], amb, c.np["shadow"], c.np["cube"],
                                3, app.pcfSearchRadius)
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), ref)


def test_c3_4k_properties(ctx, built_lib, oracle):
    """BASELINE configs[2] exactly as bench.py times it (3840x2160, blurCount 4, 3 lights, 4 x 4096^2 cascades, 256^2 cube,
    literal PCF): size-independent properties, the oracle on two bands (mid-frame; the near ground at the bottom, where the
    SSAO tap discs are widest) and -- on a many-core host such as the GPU box's -- on the WHOLE frame."""
    import os
    from crychic_renderer_amd import Crychic
    W, H = 3840, 2160
    c = get_case(ctx, built_lib, W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
    lib, check = built_lib.lib, built_lib.check
    app = Crychic(ctx, W, H, c.dev["randvec"], c.dev["cube"], shadow_dim=4096)
    app.load_scene({**c.dev, "consts": c.consts})
    app.blurCount, app.numDirLights = 4, 3
    app.Draw()
    torch.cuda.synchronize()
    full = app.mBackBuffer.cpu().numpy().copy()
    ao = dev_u16(app.mSsao.mAmbientMap0).copy()
    # (1) idempotence / determinism: a second draw gives the same bytes
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), full)
    # (2) strip decomposition (8 ranks) == whole frame
    app.mBackBuffer.zero_()
    for rank in range(8):
        r0, rn = C.c_uint32(), C.c_uint32()
        check(lib.crychic_strip_rows(H, 8, rank, C.byref(r0), C.byref(rn)))
        app.mSsao.mAmbientMap0.fill_(0x5A5A)
        app.Draw(r0.value, rn.value)
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), full)
    # (3) blur of a constant map is the identity
    check(lib.crychic_ssao_edges(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]),
                                 ptr(c.edge), W, H, 0, H // 2, stream(ctx)))
    c.a0.fill_(12345)
    for horz in (1, 0):
        check(lib.crychic_ssao_blur(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.edge), ptr(c.a0), ptr(c.a1), W, H, horz, 0,
                                    H // 2, stream(ctx)))
        torch.cuda.synchronize()
        assert int((c.a1 != 12345).sum()) == 0
    # (4) uncovered pixels carry the clear colour, covered ones alpha 255
    cov = c.np["depth"] < 0xFFFFFF
    assert (full[~cov] == np.array([176, 196, 222, 255], dtype=np.uint8)).all()
    assert (full[cov][:, 3] == 255).all()
    # (5) oracle on bands of rows (SSAO rows via the oracle's row range): mid-frame and the near ground at the bottom
    check(lib.crychic_ssao(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]),
                           ptr(c.dev["randvec"]), ptr(c.a0), ptr(c.edge), W, H, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    raw_ssao = dev_u16(c.a0).copy()
    for band0, band1 in ((H // 2 - 24, H // 2 + 24), (H - 64, H)):
        ref_ssao = oracle.ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], band0 // 2, (band1 - band0) // 2)
        assert np.array_equal(raw_ssao[band0 // 2:band1 // 2], ref_ssao[band0 // 2:band1 // 2]), (band0, band1)
        ref_band = oracle.deferred_light(c.pcb, c.np["g0"], c.np["g1"], c.np["g2"], c.np["depth"], ao, c.np["shadow"], c.np["cube"],
                                         3, app.pcfSearchRadius, row0=band0, rows=band1 - band0)
        assert np.array_equal(full[band0:band1], ref_band[band0:band1]), (band0, band1)
    # (6) the whole frame against the oracle where the host can afford it (128 cores: ~1 s)
    if (os.cpu_count() or 1) >= 32:
        ref_ao = oracle.compute_ssao(c.scb, c.np["normal"], c.np["depth"], c.np["randvec"], 4)
        assert np.array_equal(ao, ref_ao), "AO differs in %d texels" % int((ao != ref_ao).sum())
        ref = oracle.deferred_light(c.pcb, c.np["g0"], c.np["g1"], c.np["g2"], c.np["depth"], ref_ao, c.np["shadow"], c.np["cube"],
                                    3, app.pcfSearchRadius)
        assert np.array_equal(full, ref), "frame differs in %d bytes" % int((full != ref).sum())
        # the evidently intended PCF (2.5-texel rotated Poisson disc), whole frame as well
        app.pcfSearchRadius = lib.crychic_pcf_search_radius(4096, 0)
        app.Draw()
        torch.cuda.synchronize()
        ref = oracle.deferred_light(c.pcb, c.np["g0"], c.np["g1"], c.np["g2"], c.np["depth"], ref_ao, c.np["shadow"], c.np["cube"],
                                    3, app.pcfSearchRadius)
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), ref)


def test_c3_4k_covered_camera_whole_frame(ctx, built_lib, oracle):
    """The benchmark's covered-camera leg (bench.py config.camera_covered: camera pitched down until no pixel is sky, so none of
    the sky exits fires and every G-buffer texel is read), 3840x2160, blurCount 4, 3 lights, 4 x 4096^2 cascades: the whole frame
    against the oracle on a many-core host (the GPU box's), two bands of it elsewhere."""
    import os
    from crychic_renderer_amd import Crychic, scene
    W, H = 3840, 2160
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device),
                              consts=scene.Constants(W, H, 4096, cam=scene.covered_camera(W, H)))
    p = scene_util.np_planes(planes)
    consts = planes["consts"]
    assert ((p["depth"] & 0xFFFFFF) != 0xFFFFFF).all()
    scb = oracle_lib.as_oracle_cb(consts.ssao_cb, oracle_lib.OrSsaoConstants)
    pcb = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
    app.load_scene(planes)
    app.blurCount, app.numDirLights = 4, 3
    app.Draw()
    torch.cuda.synchronize()
    full = app.mBackBuffer.cpu().numpy()
    ao = dev_u16(app.mSsao.mAmbientMap0)
    if (os.cpu_count() or 1) >= 32:
        ref_ao = oracle.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 4)
        assert np.array_equal(ao, ref_ao), "AO differs in %d texels" % int((ao != ref_ao).sum())
        ref = oracle.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], ref_ao, p["shadow"], p["cube"], 3, app.pcfSearchRadius)
        assert np.array_equal(full, ref), "frame differs in %d bytes" % int((full != ref).sum())
    else:
        for band0, band1 in ((H // 2 - 16, H // 2 + 16), (H - 32, H)):
            ref_ssao = oracle.ssao(scb, p["normal"], p["depth"], p["randvec"], band0 // 2, (band1 - band0) // 2)
            check = built_lib.check
            a = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=ctx.device)
            check(built_lib.lib.crychic_ssao(ctx.handle, C.byref(consts.ssao_cb), ptr(planes["normal"]), ptr(planes["depth"]), ptr(planes["randvec"]),
                                             ptr(a), ptr(app.mSsao.mEdge), W, H, band0 // 2, (band1 - band0) // 2, stream(ctx)))
            torch.cuda.synchronize()
            assert np.array_equal(dev_u16(a)[band0 // 2:band1 // 2], ref_ssao[band0 // 2:band1 // 2])
            ref_band = oracle.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], ao, p["shadow"], p["cube"], 3, app.pcfSearchRadius,
                                             row0=band0, rows=band1 - band0)
            assert np.array_equal(full[band0:band1], ref_band[band0:band1])


@pytest.mark.parametrize("seed", [0, 1, 3, 12, 13, 15, 18])
def test_sky_shortcut_on_device(ctx, built_lib, oracle, seed):
    """The SSAO sky shortcut on the device (wave-level skip driven by the coarse geometry map of depth_pairs_kernel) against the
    oracle, on the probe frames of tests/test_hostsim_parity.py::test_sky_shortcut_is_exact; run twice on the same workspace so
    that a stale geometry map from the previous frame can only make the second run more conservative, never wrong."""
    import fuzz_util
    W, H, c, scb, depth, normal, randvec = fuzz_util.sky_probe_case(seed)
    lib, check = built_lib.lib, built_lib.check
    dev = ctx.device
    d = torch.from_numpy(depth.view(np.int32)).to(dev); n = torch.from_numpy(normal).to(dev); r = torch.from_numpy(randvec).to(dev)
    a0 = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=dev)
    edge = torch.zeros((int(lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=dev)
    ref = oracle.ssao(scb, normal, depth, randvec)
    check(lib.crychic_ssao(ctx.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(edge), W, H, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    assert np.array_equal(dev_u16(a0), ref)
    # next frame on the same workspace: the sky and the geometry swap sides of the frame
    depth2 = np.ascontiguousarray(depth[:, ::-1]); normal2 = np.ascontiguousarray(normal[:, ::-1])
    d.copy_(torch.from_numpy(depth2.view(np.int32))); n.copy_(torch.from_numpy(normal2))
    ref2 = oracle.ssao(scb, normal2, depth2, randvec)
    check(lib.crychic_ssao(ctx.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(edge), W, H, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    assert np.array_equal(dev_u16(a0), ref2)
    # the whole ComputeSsao chain on these frames: the record sweeps take their unoccluded-tile exit next to occluded patches
    a1 = torch.zeros_like(a0)
    for blur_count in (2, 5):
        check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.ssao_cb), ptr(n), ptr(d), ptr(r), ptr(a0), ptr(a1), ptr(edge), W, H, blur_count, 0,
                                       H // 2, stream(ctx)))
        torch.cuda.synchronize()
        assert np.array_equal(dev_u16(a0), oracle.compute_ssao(scb, normal2, depth2, randvec, blur_count)), blur_count


def test_flat_wall_ssao_is_unoccluded(ctx, built_lib):
    """a flat plane facing the camera has distZ = 0 <= eps for every tap => access = 1."""
    W, H = 128, 128
    c = get_case(ctx, built_lib, 64, 64)
    consts = scene_util.cpu_scene(W, H, 512, 64)["consts"]
    depth = torch.full((H, W), int(round(0.5 * 16777215)), dtype=torch.int32, device=ctx.device)
    normal = torch.zeros((H, W, 4), dtype=torch.float16, device=ctx.device)
    normal[..., 2] = -1.0
    a = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=ctx.device)
    built_lib.check(built_lib.lib.crychic_ssao(ctx.handle, C.byref(consts.ssao_cb), ptr(normal), ptr(depth), ptr(c.dev["randvec"]),
                                               ptr(a), None, W, H, 0, H // 2, stream(ctx)))
    torch.cuda.synchronize()
    inner = dev_u16(a)[8:-8, 8:-8]  # away from the border (taps that leave the map see depth 1.0)
    assert (inner == 65535).all()


def test_error_behaviour(ctx, built_lib):
    """Argument errors come back as negative status + message (the reference throws DxException)."""
    lib = built_lib.lib
    c = get_case(ctx, built_lib, 64, 64)
    rc = lib.crychic_ssao(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]), ptr(c.dev["randvec"]),
                          ptr(c.a0), None, 63, 64, 0, 32, stream(ctx))
    assert rc == -1 and b"even" in lib.crychic_last_error()
    rc = lib.crychic_ssao(ctx.handle, C.byref(c.consts.ssao_cb), None, ptr(c.dev["depth"]), ptr(c.dev["randvec"]), ptr(c.a0), None,
                          64, 64, 0, 32, stream(ctx))
    assert rc == -1
    rc = lib.crychic_ssao_blur(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.edge), ptr(c.a0), ptr(c.a0), 64, 64, 1, 0, 32, stream(ctx))
    assert rc == -1 and b"in place" in lib.crychic_last_error()
    rc = lib.crychic_ssao(ctx.handle, C.byref(c.consts.ssao_cb), ptr(c.dev["normal"]), ptr(c.dev["depth"]), ptr(c.dev["randvec"]),
                          ptr(c.a0), None, 64, 64, 30, 8, stream(ctx))
    assert rc == -1
    with pytest.raises(built_lib.CrychicError):
        built_lib.check(rc)
