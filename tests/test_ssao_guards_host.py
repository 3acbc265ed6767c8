"""CPU tier of the guard sweep (tests/ssao_guard_cases.py): every host guard of the SSAO pass and the blur chain driven across its
threshold.  Per case the guards -- read from the product's own functions through hs_ssao_guards, never restated -- must decide what
the table says, the kernel bodies with every shortcut the guards allow must equal the oracle (which has no shortcut) bit for bit,
whole map and row strips, and the shortcut counters must be non-zero where the table says they bite and exactly zero where the
guard is off.  The device tier (tests/test_ssao_guards_gpu.py) repeats the comparison through the C ABI."""
import numpy as np
import pytest

import fuzz_util
import oracle_lib
import ssao_guard_cases as G


def check_frame_is_not_degenerate(case, raw, blurred=None):
    """A frame generated for another projection comes out all 65535 and compares nothing: the table may hold no such case."""
    assert int((raw < 65535).sum()) > 50 and int((raw == 65535).sum()) > 50, (case.name, int((raw < 65535).sum()), int((raw == 65535).sum()))
    if case.blur and blurred is not None:
        assert int((blurred != raw).sum()) > 50, case.name


@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_guard_case_on_host(built_lib, oracle, hostsim, case):
    f = G.build_frame(case)
    decided = hostsim.ssao_guards(f.cb, f.W, f.H)
    assert {g: decided[g] for g in G.GUARDS} == case.expect
    assert (decided["rx"] >= 8 and decided["ry"] >= 8) if decided["sky"] else (decided["rx"], decided["ry"]) == (0, 0)
    scb = oracle_lib.as_oracle_cb(f.cb, oracle_lib.OrSsaoConstants)
    eb = int(built_lib.lib.crychic_edge_plane_bytes(f.W, f.H))
    raw = oracle.ssao(scb, f.normal, f.depth, f.randvec)
    want = oracle.compute_ssao(scb, f.normal, f.depth, f.randvec, G.BLUR_COUNT)
    check_frame_is_not_degenerate(case, raw, want)
    got, _ = hostsim.ssao(f.cb, f.normal, f.depth, f.randvec, eb)
    counters = {"sky_waves": int(hostsim.lib.hs_last_sky_waves()), "culled_taps": int(hostsim.lib.hs_last_culled_taps()),
                "clear_cell_taps": int(hostsim.lib.hs_last_clear_cell_taps())}
    assert np.array_equal(got, raw), int((got != raw).sum())
    for row0, rows in G.strips(f.H):
        part, _ = hostsim.ssao(f.cb, f.normal, f.depth, f.randvec, eb, row0=row0, rows=rows)
        assert np.array_equal(part[row0:row0 + rows], raw[row0:row0 + rows]), (row0, rows)
    got, _ = hostsim.compute_ssao(f.cb, f.normal, f.depth, f.randvec, eb, G.BLUR_COUNT)
    counters["settled_tiles"] = int(hostsim.lib.hs_last_settled_tiles())
    assert np.array_equal(got, want), int((got != want).sum())
    for row0, rows in G.strips(f.H):
        part, _ = hostsim.compute_ssao(f.cb, f.normal, f.depth, f.randvec, eb, G.BLUR_COUNT, row0, rows)
        assert np.array_equal(part[row0:row0 + rows], want[row0:row0 + rows]), (row0, rows)
    for name in case.bites:
        assert counters[name] > 0, (name, counters)
    for name in case.must_be_zero:
        assert counters[name] == 0, (name, counters)


def test_table_visits_both_sides_of_every_guard(hostsim):
    """Over the table every guard output took both values -- as the product's functions decide, and as the table expects -- and for
    every shortcut counter some case demands that it bites and some case demands that it stays at zero."""
    seen = {g: set() for g in G.GUARDS}
    for case in G.CASES:
        c = G.case_constants(case)
        W, H = G.FRAME_SIZE[case.frame]
        decided = hostsim.ssao_guards(c.ssao_cb, W, H)
        for g in G.GUARDS:
            assert decided[g] == case.expect[g], (case.name, g)
            seen[g].add(decided[g])
    assert all(v == {0, 1} for v in seen.values()), seen
    for name in G.COUNTERS:
        assert any(name in case.bites for case in G.CASES) and any(name in case.must_be_zero for case in G.CASES), name
    # nothing a case writes reaches another: a fresh reference buffer is still the reference
    ref = G.case_constants(G.CASES[0]).ssao_cb
    assert G.CASES[0].name == "proj_reference" and ref.SurfaceEpsilon == np.float32(0.05) and not np.isnan(np.ctypeslib.as_array(ref.OffsetVectors)).any()


# ---- fuzz_util's builders: the default arguments still give the frames they gave before they took a camera ----------------------------
def _old_sky_probe_case(seed):
    from crychic_renderer_amd import scene
    rng = np.random.default_rng(1000 + seed)
    W, H = int(rng.choice([640, 770, 1024])), int(rng.choice([384, 400, 512]))
    c = scene.Constants(W, H, shadow_dim=64)
    A, B = c.ssao_cb.Proj[10], c.ssao_cb.Proj[11]
    depth = np.full((H, W), 0xFFFFFF, dtype=np.uint32)
    normal = np.zeros((H, W, 4), dtype=np.float16); normal[..., 2] = -1.0
    if seed % 2:
        normal[..., :3] = rng.standard_normal((H, W, 3)).astype(np.float16)
    for _ in range(int(rng.integers(1, 5))):
        pw, ph = int(rng.integers(1, 24)), int(rng.integers(1, 16))
        x0, y0 = int(rng.integers(0, W - pw)), int(rng.integers(0, H - ph))
        if seed >= 12:
            pw, ph = int(rng.integers(1, 3)), int(rng.integers(1, 3))
            x0 = min(W - pw, 128 * int(rng.integers(1, W // 128)) - 2 - int(rng.integers(0, 2)) * pw)
            y0 = min(H - ph, 32 * int(rng.integers(1, H // 32)) - int(rng.integers(0, 2)) * ph)
        vz = rng.uniform(99.0, 99.999, size=(ph, pw))
        zndc = A + B / vz
        depth[y0:y0 + ph, x0:x0 + pw] = np.round(zndc * 16777215.0).astype(np.uint32)
        normal[y0:y0 + ph, x0:x0 + pw, :3] = rng.standard_normal((ph, pw, 3)).astype(np.float16)
    if seed % 4 == 3:
        normal[rng.random((H, W)) < 0.01, 0] = np.inf
    randvec = rng.integers(0, 256, size=(256, 256, 4), dtype=np.uint8)
    if seed >= 12:
        randvec = (rng.integers(0, 2, size=(256, 256, 4), dtype=np.uint8) * 255).astype(np.uint8)
    return W, H, c, depth, normal, randvec


def _old_clear_cell_probe_case(seed):
    W, H, c, depth, normal, randvec = _old_sky_probe_case(seed)
    rng = np.random.default_rng(77 + seed)
    A, B = c.ssao_cb.Proj[10], c.ssao_cb.Proj[11]
    x0, x1 = W // 5, W // 5 + 90 + 8 * seed
    vz = rng.uniform(1.0, 1.8, size=(H // 2, x1 - x0))
    depth[H // 4:H // 4 + H // 2, x0:x1] = np.clip(np.round((A + B / vz) * 16777215.0), 0, 0xFFFFFF).astype(np.uint32)
    normal[H // 4:H // 4 + H // 2, x0:x1, :3] = rng.standard_normal((H // 2, x1 - x0, 3)).astype(np.float16)
    normal[rng.random((H, W)) < 0.002, 1] = np.nan
    c.ssao_cb.OcclusionRadius = 3.0
    return W, H, c, depth, normal, randvec


def _old_rough_wall_case(seed, W, H, sky_blocks):
    from crychic_renderer_amd import scene
    rng = np.random.default_rng(seed)
    c = scene.Constants(W, H, shadow_dim=64)
    A, B = c.ssao_cb.Proj[10], c.ssao_cb.Proj[11]
    vz = rng.uniform(6.0, 6.6, size=(H, W))
    depth = np.clip(np.round((A + B / vz) * 16777215.0), 0, 0xFFFFFE).astype(np.uint32)
    normal = np.zeros((H, W, 4), np.float16); normal[..., 2] = -1.0
    normal[..., :2] = (0.5 * rng.standard_normal((H, W, 2))).astype(np.float16)
    randvec = rng.integers(0, 256, size=(256, 256, 4), dtype=np.uint8)
    if sky_blocks:
        rng = np.random.default_rng(100 + seed)
        for by in range(0, H, 96):
            for bx in range(0, W, 256):
                if rng.random() < 0.5:
                    depth[by:by + 96, bx:bx + 256] = 0xFFFFFF
                    normal[by:by + 96, bx:bx + 256, :3] = (0, 0, -1)
    return c, depth, normal, randvec


def _old_cull_probe_case(seed, W=256, H=160):
    import scene_util
    pl = scene_util.cpu_scene(W, H, 64, 8)
    p = scene_util.np_planes(pl)
    rng = np.random.default_rng(1234 + seed)
    depth, normal = p["depth"].copy(), p["normal"].copy()
    n = 60
    ys, xs = rng.integers(0, H, n), rng.integers(0, W, n)
    kind = rng.integers(0, 4, n)
    base = depth[ys, xs] & 0xFFFFFF
    spike = np.where(kind == 0, rng.integers(0, 1 << 22, n),
            np.where(kind == 1, base - rng.integers(0, 200, n).clip(max=base),
            np.where(kind == 2, 0xFFFFFF, 0))).astype(np.uint32)
    depth[ys, xs] = spike
    for _ in range(6):
        y0, x0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 4))
        depth[y0:y0 + int(rng.integers(1, 5)), x0:x0 + int(rng.integers(1, 5))] = int(rng.integers(0, 1 << 24))
    normal[rng.integers(0, H, 40), rng.integers(0, W, 40), 0] = np.nan
    return depth, normal, p["randvec"]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_cb(a, b):
    import ctypes as C
    return bytes(C.string_at(C.addressof(a), C.sizeof(a))) == bytes(C.string_at(C.addressof(b), C.sizeof(b)))


def test_default_builders_are_unchanged(built_lib):
    """Without consts= / cam= the four builders reproduce, byte for byte, the arrays (and constants) of the arithmetic they had
    before the wall and the patches were placed relative to the camera -- the old arithmetic is kept above."""
    W, H, c, scb, depth, normal, randvec = fuzz_util.sky_probe_case(15)
    oW, oH, oc, odepth, onormal, orandvec = _old_sky_probe_case(15)
    assert (W, H) == (oW, oH) and same_cb(c.ssao_cb, oc.ssao_cb)
    assert same_bytes(depth, odepth) and same_bytes(normal, onormal) and same_bytes(randvec, orandvec)
    W, H, c, scb, depth, normal, randvec = fuzz_util.clear_cell_probe_case(3)
    oW, oH, oc, odepth, onormal, orandvec = _old_clear_cell_probe_case(3)
    assert (W, H) == (oW, oH) and same_cb(c.ssao_cb, oc.ssao_cb)
    assert same_bytes(depth, odepth) and same_bytes(normal, onormal) and same_bytes(randvec, orandvec)
    c, scb, depth, normal, randvec = fuzz_util.rough_wall_case(3, 322, 190, True)
    oc, odepth, onormal, orandvec = _old_rough_wall_case(3, 322, 190, True)
    assert same_cb(c.ssao_cb, oc.ssao_cb) and same_bytes(depth, odepth) and same_bytes(normal, onormal) and same_bytes(randvec, orandvec)
    W, H, c, depth, normal, randvec = fuzz_util.cull_probe_case(3)
    odepth, onormal, orandvec = _old_cull_probe_case(3)
    assert same_bytes(depth, odepth) and same_bytes(normal, onormal) and same_bytes(randvec, orandvec)
    assert c.ssao_cb.SurfaceEpsilon == np.float32(0.05)
