"""crychic_antialias on the CPU tier: the kernel body (csrc/post_aa_core.hpp, built for the host with the workgroup and lane walk
emulated, both the 16-byte and the dword path) against the checker (tests/post_aa_ref, plain C from the definition), byte for byte on
the whole corpus; the definition's known answers; every branch of the definition taken; row ranges; and the refusals of the real
library, which need no device."""
import ctypes as C

import numpy as np
import pytest

import post_aa_host_lib as host
import post_aa_lib as aa


def run_host(img, params=None, row0=0, rows=None, path=host.AUTO, misalign=0):
    """The kernel body on guarded copies of `img`: (out, path taken); asserts the guard bytes around both planes."""
    sraw, src = aa.guarded(img.shape, misalign=misalign)
    oraw, out = aa.guarded(img.shape, misalign=misalign)
    src[...] = img
    taken = host.antialias(src, out, params, row0, rows, path)
    assert aa.guards_intact(sraw, src) and aa.guards_intact(oraw, out), "guard bytes changed"
    assert np.array_equal(src, img), "the input plane changed"
    return out, taken


@pytest.mark.parametrize("pname", list(aa.PARAM_SETS))
def test_host_body_equals_checker(oracle, pname):
    for name, img in aa.corpus(oracle):
        ref, _ = aa.expected(name, img, pname)
        got, taken = run_host(img, aa.PARAM_SETS[pname])
        assert taken == (host.VECTOR if img.shape[1] % 4 == 0 else host.SCALAR), name
        assert np.array_equal(got, ref), "%s / %s: %d bytes differ (launcher's path)" % (name, pname, int((got != ref).sum()))
        if taken == host.VECTOR:            # the dword path on the same frame, and on a plane that is only 4-byte aligned
            got, taken = run_host(img, aa.PARAM_SETS[pname], path=host.SCALAR)
            assert taken == host.SCALAR and np.array_equal(got, ref), "%s / %s: dword path" % (name, pname)
            got, taken = run_host(img, aa.PARAM_SETS[pname], misalign=4)
            assert taken == host.SCALAR and np.array_equal(got, ref), "%s / %s: misaligned plane" % (name, pname)


def test_vector_path_needs_alignment_and_width():
    img = np.zeros((8, 8, 4), np.uint8)
    _, src = aa.guarded(img.shape, misalign=4)
    _, out = aa.guarded(img.shape, misalign=4)
    assert host.antialias(src, out, path=host.VECTOR) == -1
    odd = np.zeros((8, 6, 4), np.uint8)
    _, src = aa.guarded(odd.shape)
    _, out = aa.guarded(odd.shape)
    assert host.antialias(src, out, path=host.VECTOR) == -1


def test_known_answers():
    rng = np.random.default_rng(5)
    for fn in (lambda i: aa.checker(i)[0], lambda i: run_host(i)[0], lambda i: run_host(i, path=host.SCALAR)[0]):
        flat = np.full((24, 40, 4), 201, np.uint8)
        assert np.array_equal(fn(flat), flat)
        quiet = aa.below_threshold(40, 24, rng)
        assert quiet.min() != quiet.max() and np.array_equal(fn(quiet), quiet)
        for vertical in (True, False):
            img = aa.straight_edge(40, 24, vertical)
            got = fn(img)
            a, b = (got, img) if vertical else (got.transpose(1, 0, 2), img.transpose(1, 0, 2))     # the edge between columns m - 1 and m
            m = b.shape[1] // 2
            keep = np.ones(b.shape[1], bool)
            keep[m - 1:m + 1] = False
            assert np.array_equal(a[:, keep], b[:, keep]), "a pixel away from the edge changed"
            w = 12
            dark, light = (0 * (256 - w) + 255 * w + 128) >> 8, (255 * (256 - w) + 0 * w + 128) >> 8
            assert (a[:, m - 1, :3] == dark).all() and (a[:, m, :3] == light).all() and (a[..., 3] == 255).all()


def test_every_branch_is_taken(oracle):
    total = dict.fromkeys(aa.COUNTERS, 0)
    for name, img in aa.corpus(oracle):
        _, n = aa.expected(name, img, "default")
        assert sum(n[k] for k in ("early_copy", "horizontal", "vertical")) == img.shape[0] * img.shape[1], name
        assert n["side_a"] + n["side_b"] == n["neg_hit"] + n["neg_k"] == n["pos_hit"] + n["pos_k"] == n["horizontal"] + n["vertical"], name
        for k in total:
            total[k] += n[k]
    assert all(v > 0 for v in total.values()), total


def test_searches_reach_k_on_a_slanted_edge_and_stop_at_once_in_noise(oracle):
    images = dict(aa.corpus(oracle))
    _, n = aa.expected("slant5_h0_130x70", images["slant5_h0_130x70"], "default")
    assert n["neg_k"] > 0 and n["pos_k"] > 0
    _, n = aa.expected("noise_130x70", images["noise_130x70"], "default")
    assert n["neg_hit"] > n["neg_k"] and n["horizontal"] + n["vertical"] > n["early_copy"]


@pytest.mark.parametrize("split", [(0, 1, 2, 33, 34, 69, 70), (0, 31, 32, 70), (0, 17, 70), (0, 70)])
@pytest.mark.parametrize("path", [host.AUTO, host.SCALAR])
def test_row_ranges_stitch_to_the_whole_frame(oracle, split, path):
    images = dict(aa.corpus(oracle))
    for name, W in (("noise_130x70", 130), ("slant5_v1_130x70", 130)):
        img = images[name]
        whole, _ = aa.expected(name, img, "default")
        stitched = np.full(img.shape, aa.GUARD, np.uint8)
        for row0, end in zip(split[:-1], split[1:]):
            got, _ = run_host(img, row0=row0, rows=end - row0, path=path)
            ref, _ = aa.checker(img, row0=row0, rows=end - row0)
            assert np.array_equal(got, ref), (name, row0, end)
            assert (got[:row0] == aa.GUARD).all() and (got[end:] == aa.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = got[row0:end]
        assert np.array_equal(stitched, whole), name
    # a multiple-of-4 width takes the 16-byte path under AUTO
    img = images["rects_64x32"]
    whole, _ = aa.expected("rects_64x32", img, "default")
    for row0, rows in ((0, 1), (1, 1), (5, 20), (31, 1)):
        got, _ = run_host(img, row0=row0, rows=rows, path=path)
        assert np.array_equal(got[row0:row0 + rows], whole[row0:row0 + rows]) and (got[:row0] == aa.GUARD).all() and (got[row0 + rows:] == aa.GUARD).all()


def test_a_call_reads_only_the_rows_it_may(oracle):
    """Rows of `in` beyond 16 of the range may hold anything: the range's output does not depend on them."""
    img = dict(aa.corpus(oracle))["noise_130x70"]
    whole, _ = aa.expected("noise_130x70", img, "default")
    other = img.copy()
    other[:20 - 16] ^= 0xFF
    other[20 + 9 + 16:] ^= 0xFF
    got, _ = run_host(other, row0=20, rows=9)
    assert np.array_equal(got[20:29], whole[20:29])


def test_default_params(built_lib):
    p = built_lib.AAParams()
    assert C.sizeof(p) == 16 and built_lib.lib.crychic_aa_default_params(C.byref(p)) == 0
    assert (p.absMin, p.relShift, p.searchSteps, p.subpix) == tuple(aa.DEFAULTS[k] for k in ("absMin", "relShift", "searchSteps", "subpix"))
    assert built_lib.lib.crychic_aa_default_params(None) == -1
    assert built_lib.AA_MAX_SEARCH == 16


def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, P = built_lib.lib, built_lib.AAParams
    a, b = 0x10000000, 0x20000000           # never dereferenced

    def call(src=a, dst=b, W=64, H=32, row0=0, rows=32, params=None):
        rc = lib.crychic_antialias(None, src, dst, W, H, row0, rows, None if params is None else C.byref(params), None)
        return rc, lib.crychic_last_error().decode()
    assert call() == (-1, "null context")
    assert call(params=P(0, 31, 16, 256)) == (-1, "null context") and call(params=P(0xFFFFFFFF, 0, 1, 0)) == (-1, "null context")
    assert call(row0=32, rows=0) == (-1, "null context") and call(W=1, H=1, rows=1) == (-1, "null context")
    for kw, word in ((dict(src=None), "null argument"), (dict(dst=None), "null argument"), (dict(W=0), "non-zero"), (dict(H=0, rows=0), "non-zero"),
                     (dict(row0=33, rows=0), "outside the 32-row frame"), (dict(row0=1, rows=32), "outside the 32-row frame"),
                     (dict(row0=0xFFFFFFFF, rows=2), "outside the 32-row frame"),
                     (dict(params=P(2048, 32, 12, 192)), "relShift"), (dict(params=P(2048, 3, 0, 192)), "searchSteps"),
                     (dict(params=P(2048, 3, 17, 192)), "searchSteps"), (dict(params=P(2048, 3, 12, 257)), "subpix"),
                     (dict(dst=a), "overlap"), (dict(dst=a + 64 * 32 * 4 - 4), "overlap"), (dict(src=b + 64 * 32 * 4 - 4), "overlap"),
                     (dict(src=a + 2), "aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert call(dst=a + 64 * 32 * 4) == (-1, "null context")          # adjacent planes do not overlap
    rc, msg = call(W=1 << 15, H=1 << 14, rows=1)
    assert rc == -4 and "exceeds" in msg
