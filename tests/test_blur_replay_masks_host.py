"""The split replay body (csrc/blur_tiles.hpp: blur_replay_fetch_masks, then blur_replay_rows and blur_replay_cols with a lane's
six decision words in registers -- what blur_replay_chain_kernel runs) on the host against blur_replay_tile and the oracle, on the
frames of tests/blur_masks_lib.py: the same bits for every blurCount, for strips whose rows cut tiles, at the top and bottom edges
(rows CLAMPed into the map), at x = 0 and at ragged right edges.  CPU tier: tests/hostsim/blur_masks.cpp."""
import numpy as np
import pytest

import blur_masks_lib

CASES = [("322x190", 2), ("322x190", 4), ("128x64", 3), ("260x70", 4), ("260x70", 9), ("512x416", 2), ("sky", 2), ("sky", 3), ("sky", 4)]


@pytest.fixture(scope="module")
def bm():
    return blur_masks_lib.load()


_frames = {}


def get_frame(name):
    if name not in _frames:
        _frames[name] = blur_masks_lib.frame(name)
    return _frames[name]


@pytest.mark.parametrize("name,blur_count", CASES)
def test_split_body_equals_replay_tile_and_oracle(built_lib, oracle, hostsim, bm, name, blur_count):
    """Whole frame: split body == blur_replay_tile == oracle.compute_ssao, every texel (tiles at y = 0 and at the last, partly
    filled tile row stage CLAMPed rows; tiles at x = 0 and at the ragged right edge CLAMPed columns)."""
    W, H, c, scb, depth, normal, randvec = get_frame(name)
    eb = int(built_lib.lib.crychic_edge_plane_bytes(W, H))
    want = oracle.compute_ssao(scb, normal, depth, randvec, blur_count)
    old, settled_old = bm.compute_ssao(hostsim, c.ssao_cb, normal, depth, randvec, eb, blur_count, body=0)
    new, settled = bm.compute_ssao(hostsim, c.ssao_cb, normal, depth, randvec, eb, blur_count, body=1)
    assert np.array_equal(old, want), int((old != want).sum())
    assert np.array_equal(new, want), int((new != want).sum())
    assert np.array_equal(settled, settled_old)
    if name != "sky":
        assert settled.sum() == 0 and (want != 65535).mean() > 0.5          # every tile replays, and the blur has something to do
    elif blur_count == 2:
        assert all(n >= 1 for n in blur_masks_lib.pair_cases(settled)), blur_masks_lib.pair_cases(settled)


@pytest.mark.parametrize("name,blur_count,row0,rows", [("322x190", 4, 37, 20), ("512x416", 4, 37, 20), ("260x70", 3, 17, 5), ("sky", 4, 100, 61),
                                                       ("322x190", 9, 0, 7)])
def test_split_body_on_strips(built_lib, oracle, hostsim, bm, name, blur_count, row0, rows):
    """Row strips that cut tiles.  (37, 20) with blurCount 4: the replayed iterations owe rows 27 .. 66, 32 .. 61 and 37 .. 56, so
    tile rows 1 and 4 are in the launch and own no row of the last iteration."""
    W, H, c, scb, depth, normal, randvec = get_frame(name)
    eb = int(built_lib.lib.crychic_edge_plane_bytes(W, H))
    want = oracle.compute_ssao(scb, normal, depth, randvec, blur_count)
    old, _ = bm.compute_ssao(hostsim, c.ssao_cb, normal, depth, randvec, eb, blur_count, body=0, row0=row0, rows=rows)
    new, _ = bm.compute_ssao(hostsim, c.ssao_cb, normal, depth, randvec, eb, blur_count, body=1, row0=row0, rows=rows)
    assert np.array_equal(new[row0:row0 + rows], want[row0:row0 + rows])
    assert np.array_equal(new, old)                    # the junk outside the strip's rows included: the same texels are written


@pytest.mark.parametrize("name,blur_count", [("322x190", 3), ("260x70", 2), ("sky", 2)])
def test_apron_columns_decision_words_are_not_used(built_lib, oracle, hostsim, bm, name, blur_count):
    """While a tile replays, the decision words of its ten apron columns read 0xFFFFFFFF (all 11 taps of both sweeps accepted,
    which the rough wall's recorded words almost never are) or 0x80000000 (no tap of either sweep, not even the centre); they are the
    neighbours' own columns, so the harness restores them after the tile.  The split body gives the oracle's map all the same:
    no word of an apron column reaches a result.  (It cannot show that the words are not LOADED: the six loads per lane are
    blur_replay_fetch_masks' text, and their addresses are the lane's own column by construction.)"""
    W, H, c, scb, depth, normal, randvec = get_frame(name)
    eb = int(built_lib.lib.crychic_edge_plane_bytes(W, H))
    want = oracle.compute_ssao(scb, normal, depth, randvec, blur_count)
    for poison in (0xFFFFFFFF, 0x80000000):       # 0x80000000: neither sweep's 11 bits set, and not the harness's "no poison"
        new, _ = bm.compute_ssao(hostsim, c.ssao_cb, normal, depth, randvec, eb, blur_count, body=1, poison=poison)
        assert np.array_equal(new, want), (hex(poison), int((new != want).sum()))
