"""crychic_bloom on the CPU: the kernels' bodies built for the host (tests/bloom_host) against the checker (tests/bloom_ref) byte for
byte, every pyramid level and the frame, on the corpus, behind guard bytes and on misaligned planes; that the corpus reaches every
branch of the definition; the seven known answers of include/crychic_hip.h; row ranges; the workspace layout; and the refusals of the
C ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

import bloom_host_lib as host
import bloom_lib as bl


@pytest.fixture(scope="module")
def cases(built_lib):
    return bl.corpus()


def run_host(img, params=None, row0=0, rows=None, misalign=0, in_place=False, levels_only=False):
    """The host bodies on guarded copies of `img`; returns (frame, [U_k], stats), the guards, the input and the workspace's gaps
    checked.  The workspace is guarded and filled with 0xA5: what is not a level must stay that."""
    H, W = img.shape[:2]
    p = dict(bl.DEFAULTS, **(params or {}))
    _, need = bl.level_offsets(W, H, p["levels"])
    sraw, src = bl.guarded(img.shape, misalign=misalign)
    src[...] = img
    if in_place:
        oraw, out = sraw, src
    else:
        oraw, out = bl.guarded(img.shape, misalign=misalign)
    wraw, ws = bl.guarded((need,))
    stats = host.bloom(src, out, ws, params, row0=row0, rows=rows, composite=not levels_only)
    assert bl.guards_intact(sraw, src) and bl.guards_intact(oraw, out) and bl.guards_intact(wraw, ws), "guard bytes changed"
    assert (ws[~bl.written_mask(W, H, p["levels"], need)] == bl.GUARD).all(), "a workspace byte between two levels was written"
    if not in_place:
        assert np.array_equal(src, img), "the input plane changed"
    return out.copy(), [u.copy() for u in bl.split_workspace(ws, W, H, p["levels"])], stats


def assert_equal(name, got, levels, ref, ref_levels):
    assert len(levels) == len(ref_levels), name
    for k, (g, r) in enumerate(zip(levels, ref_levels), 1):
        assert np.array_equal(g, r), "%s: level %d differs in %d values" % (name, k, int((g != r).sum()))
    assert np.array_equal(got, ref), "%s: %d bytes of the frame differ" % (name, int((got != ref).sum()))


@pytest.mark.parametrize("pname", list(bl.PARAM_SETS) + ["scene"])
def test_host_bodies_equal_checker(cases, pname):
    turn, vec = 0, 0
    for name, img, pn in cases:
        if pn != pname:
            continue
        ref, ref_levels, _ = bl.expected(name)
        misalign = (0, 4, 12)[turn % 3]
        turn += 1
        got, levels, stats = run_host(img, bl.case_params(pn), misalign=misalign)
        assert_equal("%s at %d" % (name, misalign), got, levels, ref, ref_levels)
        vec += stats["vec_composites"]
        got, levels, _ = run_host(img, bl.case_params(pn), misalign=(4, 12, 0)[turn % 3], in_place=True)
        assert_equal(name + " in place", got, levels, ref, ref_levels)
    assert turn >= 1 and vec >= 1, "a parameter set without a case on 16-byte aligned planes"


def test_the_corpus_reaches_what_it_must(cases):
    total = dict.fromkeys(bl.COUNTERS, 0)
    seen = {f: set() for f in bl.FIELDS}
    deeper = 0
    for name, img, pn in cases:
        _, levels, n = bl.expected(name)
        p = bl.case_params(pn)
        for k in bl.COUNTERS:
            total[k] += n[k]
        for f in bl.FIELDS:
            seen[f].add(p[f])
        deeper += p["levels"] > len(levels)
    assert all(total[k] > 0 for k in bl.COUNTERS), total
    assert {0, 256} <= seen["scatter"] and {1, 8} <= seen["levels"] and {0, 1024} <= seen["intensity"] and {1, 255} <= seen["knee"]
    assert {0, 255} <= seen["threshold"]
    assert deeper > 0, "no case asks for more levels than its frame has"
    assert {(im.shape[1], im.shape[0]) for _, im, _ in cases} >= set(bl.SIZES)
    # the host build's own shortcuts are taken and not taken
    _, _, dark = run_host(cases[0][1], bl.PARAM_SETS["dark"], in_place=True)
    assert dark["zero_tiles"] > 0 and dark["silent_waves"] > 0
    assert bl.expected("322x190_blob_default")[2]["w_zero"] > 0
    _, _, blob = run_host({c[0]: c for c in cases}["322x190_blob_default"][1], None, in_place=True)
    assert blob["zero_tiles"] > 0 and blob["groups"] > blob["zero_tiles"], "the blob frame has tiles of zeros and tiles that are filtered"


def test_the_weight_by_multiply_high_is_the_division(built_lib):
    assert host.weight_mismatches() == 0


def answers(fn):
    """The seven known answers of the header through fn(img, params) -> (frame, [U_k])."""
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    # 1: intensity 0
    out, _ = fn(noise, dict(intensity=0, threshold=0))
    assert np.array_equal(out, noise)
    # 2: nothing over the threshold: luma at most 77 * 100 + 150 * 100 + 29 * 100 = 256 * 100
    dim = rng.integers(0, 101, (37, 53, 4), dtype=np.uint8)
    dim[0, 0, :3] = 100
    out, levels = fn(dim, dict(threshold=100, knee=1, intensity=1024))
    assert np.array_equal(out, dim) and all(not u.any() for u in levels)
    # 3: one colour over the threshold
    for c, prm in (((250, 240, 200), dict()), ((255, 255, 255), dict(intensity=1024, scatter=256)), ((10, 255, 0), dict(threshold=100, knee=7, levels=8))):
        p = dict(bl.DEFAULTS, **prm)
        L = 77 * c[0] + 150 * c[1] + 29 * c[2]
        assert L > 256 * p["threshold"]
        w = min(256, (L - 256 * p["threshold"]) // p["knee"])
        img = np.empty((45, 70, 4), np.uint8)
        img[...] = c + (77,)
        out, levels = fn(img, prm)
        assert len(levels) == min(p["levels"], 7)
        for u in levels:
            assert (u == np.array([c[0] * w, c[1] * w, c[2] * w, 0], np.uint16)).all()
        want = [min(255, ch + ((ch * w * p["intensity"] + 32768) >> 16)) for ch in c] + [77]
        assert (out == np.array(want, np.uint8)).all()
    # 4: never darker; alpha kept
    out, _ = fn(noise, dict(threshold=60, intensity=900))
    assert (out[..., :3] >= noise[..., :3]).all() and (out[..., :3] > noise[..., :3]).any() and np.array_equal(out[..., 3], noise[..., 3])
    # 5: scatter 0: the levels from the second on have no influence
    one, l1 = fn(noise, dict(threshold=60, scatter=0, levels=1))
    six, l6 = fn(noise, dict(threshold=60, scatter=0, levels=6))
    assert np.array_equal(one, six) and np.array_equal(l1[0], l6[0]) and len(l6) == 6
    lit, _ = fn(noise, dict(threshold=60, scatter=128, levels=6))
    assert not np.array_equal(lit, six)
    # 6: the eight symmetries of the square
    q = rng.integers(0, 256, (32, 32, 4), dtype=np.uint8)
    sym = np.zeros((64, 64, 4), np.uint32)
    quarter = np.zeros((64, 64, 4), np.uint8)
    quarter[:32, :32] = q
    for k in range(4):
        r = np.rot90(quarter, k)
        sym = sym + r + np.transpose(r, (1, 0, 2))
    sym = np.ascontiguousarray((sym // 2).clip(0, 255).astype(np.uint8))
    assert np.array_equal(sym, np.rot90(sym)) and np.array_equal(sym, np.transpose(sym, (1, 0, 2)))
    out, _ = fn(sym, dict(threshold=80, intensity=512))
    assert not np.array_equal(out, sym)
    for k in range(4):
        r = np.rot90(out, k)
        assert np.array_equal(r, out) and np.array_equal(np.transpose(r, (1, 0, 2)), out)
    # 7: the transpose
    out, _ = fn(noise, dict(threshold=60, intensity=512))
    outT, _ = fn(np.ascontiguousarray(np.transpose(noise, (1, 0, 2))), dict(threshold=60, intensity=512))
    assert np.array_equal(outT, np.transpose(out, (1, 0, 2)))


def test_known_answers(built_lib):
    answers(lambda img, p: bl.checker(img, p)[:2])
    answers(lambda img, p: run_host(img, p)[:2])
    answers(lambda img, p: run_host(img, p, misalign=4)[:2])


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 190), (0, 3, 190), (0, 7, 12, 95, 96, 101, 190)])
def test_row_ranges_stitch_to_the_whole_frame(cases, split):
    name = "322x190_blob_default"
    img = {c[0]: c for c in cases}[name][1]
    whole, _, _ = bl.expected(name)
    for misalign in (0, 4):
        H, W = img.shape[:2]
        _, need = bl.level_offsets(W, H, 6)
        _, src = bl.guarded(img.shape, misalign=misalign)
        src[...] = img
        wraw, ws = bl.guarded((need,))
        host.bloom(src, src, ws, composite=False)
        levels = ws.copy()
        stitched = np.full(img.shape, bl.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            oraw, out = bl.guarded(img.shape, misalign=misalign)
            host.bloom(src, out, ws, row0=row0, rows=end - row0, pyramid=False)
            assert bl.guards_intact(oraw, out) and (out[:row0] == bl.GUARD).all() and (out[end:] == bl.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = out[row0:end]
            ref_rows, _, _ = bl.checker(img, row0=row0, rows=end - row0)
            assert np.array_equal(out, ref_rows)
        assert np.array_equal(stitched, whole)
        assert np.array_equal(ws, levels) and bl.guards_intact(wraw, ws), "the composite wrote the workspace"
        oraw, out = bl.guarded(img.shape, misalign=misalign)
        host.bloom(src, out, ws, row0=190, rows=0, pyramid=False)
        assert (out == bl.GUARD).all(), "rows == 0 wrote"


def test_workspace_size_and_offsets(built_lib):
    lib = built_lib.lib
    sizes = list(bl.SIZES) + [(3840, 2160), (1920, 1080), (1, 300), (300, 1), (255, 256), (257, 2), (16384, 16384)]
    for W, H in sizes:
        for n in range(1, 9):
            offs, need = bl.level_offsets(W, H, n)
            assert lib.crychic_bloom_workspace_bytes(W, H, n) == need == host.workspace_bytes(W, H, n), (W, H, n)
            assert [lib.crychic_bloom_level_offset(W, H, n, k) for k in range(1, len(offs) + 1)] == offs, (W, H, n)
            assert all(o % 16 == 0 for o in offs)
            assert lib.crychic_bloom_level_offset(W, H, n, 0) == 0 and lib.crychic_bloom_level_offset(W, H, n, len(offs) + 1) == 0
            assert bl._ref().bloom_ref_levels(W, H, n) == len(offs)
    assert bl.level_sizes(1, 1, 8) == [(1, 1)] and bl.level_sizes(2, 1, 8) == [(1, 1)] and bl.level_sizes(3, 2, 8) == [(2, 1), (1, 1)]
    assert bl.level_sizes(3840, 2160, 8)[-1] == (15, 9) and len(bl.level_sizes(256, 256, 8)) == 8 and len(bl.level_sizes(128, 128, 8)) == 7
    assert bl.level_offsets(7, 5, 1) == ([0], 4 * 3 * 8) and bl.level_offsets(5, 5, 2) == ([0, 80], 80 + 2 * 2 * 8)
    assert lib.crychic_bloom_workspace_bytes(0, 4, 1) == 0 and lib.crychic_bloom_workspace_bytes(4, 4, 0) == 0 and lib.crychic_bloom_workspace_bytes(4, 4, 9) == 0


def test_default_params(built_lib):
    p = built_lib.BloomParams()
    assert C.sizeof(p) == 32 and built_lib.lib.crychic_bloom_default_params(C.byref(p)) == 0
    assert (p.threshold, p.knee, p.scatter, p.intensity, p.levels, list(p.reserved)) == (192, 32, 179, 128, 6, [0, 0, 0])
    assert {f: getattr(p, f) for f in bl.FIELDS} == bl.DEFAULTS
    assert built_lib.lib.crychic_bloom_default_params(None) == -1
    assert built_lib.BLOOM_MAX_LEVELS == 8 == bl.MAX_LEVELS
    q = built_lib.BloomParams.default(threshold=10, levels=3)
    assert (q.threshold, q.knee, q.levels) == (10, 32, 3)


def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, P = built_lib.lib, built_lib.BloomParams
    a, b, w = 0x10000000, 0x20000000, 0x30000000           # never dereferenced
    W, H = 64, 32
    need = bl.level_offsets(W, H, 6)[1]
    plane = W * H * 4

    def calls(src=a, dst=b, W=W, H=H, row0=0, rows=None, params=None, ws=w, size=need, only=None):
        """The three entries on the same arguments: [(rc, message)]; `only` picks entries by their position."""
        pp = None if params is None else C.byref(params)
        out = []
        if only in (None, 0):
            out.append((lib.crychic_bloom_pyramid(None, src, W, H, pp, ws, size, None), lib.crychic_last_error().decode()))
        if only in (None, 1):
            out.append((lib.crychic_bloom_composite(None, src, dst, W, H, row0, H if rows is None else rows, pp, ws, size, None),
                        lib.crychic_last_error().decode()))
        if only in (None, 2) and row0 == 0 and rows is None:
            out.append((lib.crychic_bloom(None, src, dst, W, H, pp, ws, size, None), lib.crychic_last_error().decode()))
        return out

    ok = (-1, "null context")
    assert calls() == [ok] * 3
    assert calls(dst=a) == [ok] * 3, "in == out is in place"
    assert calls(dst=a + plane) == [ok] * 3 and calls(ws=a + plane) == [ok] * 3, "adjacent ranges do not overlap"
    assert calls(row0=32, rows=0) == [ok] * 2 and calls(W=1, H=1, size=8) == [ok] * 3
    assert calls(size=need + 1000) == [ok] * 3
    edge = P.default(threshold=255, knee=255, scatter=256, intensity=1024, levels=8)
    assert calls(params=edge, size=bl.level_offsets(W, H, 8)[1]) == [ok] * 3
    assert calls(params=P.default(threshold=0, knee=1, scatter=0, intensity=0, levels=1), size=32 * 16 * 8) == [ok] * 3
    bad_res = P.default()
    bad_res.reserved[2] = 1
    for kw, word in ((dict(src=None), "null argument"), (dict(ws=None), "null argument"), (dict(src=a + 2), "4-byte aligned"),
                     (dict(ws=w + 8), "16-byte aligned"), (dict(ws=w + 4), "16-byte aligned"), (dict(W=0), "non-zero"), (dict(H=0), "non-zero"),
                     (dict(params=P.default(threshold=256)), "threshold"), (dict(params=P.default(knee=0)), "knee"), (dict(params=P.default(knee=256)), "knee"),
                     (dict(params=P.default(scatter=257)), "scatter"), (dict(params=P.default(intensity=1025)), "intensity"),
                     (dict(params=P.default(levels=0)), "levels"), (dict(params=P.default(levels=9)), "levels"), (dict(params=bad_res), "reserved"),
                     (dict(size=need - 1), "workspace has"), (dict(size=0), "workspace has"),
                     (dict(params=P.default(levels=5), size=bl.level_offsets(W, H, 5)[1] - 8), "workspace has"),
                     (dict(ws=a), "workspace overlaps"), (dict(ws=a + plane - 16), "workspace overlaps"), (dict(src=w + need - 4), "workspace overlaps")):
        got = calls(**kw)
        assert len(got) == 3 and all(rc == -1 and word in msg for rc, msg in got), (kw, got)
    for kw, word in ((dict(dst=None), "null argument"), (dict(dst=b + 1), "4-byte aligned"), (dict(dst=a + 4), "planes overlap"),
                     (dict(dst=a + plane - 4), "planes overlap"), (dict(src=b + plane - 4), "planes overlap"), (dict(ws=b), "workspace overlaps"),
                     (dict(ws=b + plane - 16), "workspace overlaps"), (dict(dst=w + need - 4), "workspace overlaps")):
        got = calls(**kw)[1:]
        assert len(got) == 2 and all(rc == -1 and word in msg for rc, msg in got), (kw, got)
    for kw in (dict(row0=33, rows=0), dict(row0=1, rows=32), dict(row0=0xFFFFFFFF, rows=2)):
        rc, msg = calls(only=1, **kw)[0]
        assert rc == -1 and "outside the 32-row frame" in msg, (kw, rc, msg)
    big = bl.level_offsets(1 << 15, (1 << 13) + 1, 6)[1]
    got = calls(W=1 << 15, H=(1 << 13) + 1, size=big, dst=a, ws=0x70000000)
    assert all(rc == -4 and "exceeds" in msg for rc, msg in got), got
    big = bl.level_offsets(1 << 15, 1 << 13, 6)[1]
    assert calls(W=1 << 15, H=1 << 13, size=big, dst=a, ws=0x70000000) == [ok] * 3        # 2^28 pixels
