"""The wave votes of the lighting kernels, CPU tier (DESIGN.md section 3 "wave votes").  On the host a vote is the lane's own
predicate, so what this tier can say of the votes is (1) that the test harness groups pixels into wavefronts as the kernels do,
(2) that the corpus of tests/light_votes_lib.py drives every vote a configuration can reach to both sides and across its boundary --
unanimous wavefronts, wavefronts refused by exactly one lane at lanes 0, 1, 31, 32, 62, 63 and the last live lane of the partial
wavefront, unanimous partial wavefronts, unanimous wavefronts over an uncovered lane that holds the spoiler -- which is the condition
under which tests/test_light_votes_gpu.py means anything, and (3) that the kernel bodies give the oracle's bits on those frames.
Tolerance: none (RGBA8 bytes; radiance bits, NaN == NaN: fuzz_util.same_floats)."""
import numpy as np
import pytest

import fuzz_util
import light_votes_lib as lv


@pytest.mark.parametrize("w", [200, 64])
@pytest.mark.parametrize("quads", [False, True])
def test_grouping_reproduces_the_kernels_footprint(w, quads):
    """wave_pixels == light_tile_pixel over grid_for's blocks, thread by thread: a row range that is no multiple of the tile height,
    anchored on a row that is no multiple of it either."""
    row0, rows = 22, 22
    nbx, nby = (w + 63) // 64, (rows + 3) // 4                      # grid_for(W, rows): 64 x 4 pixels per block of 256 threads
    want = np.full((nby * nbx * 4, 64), -1, np.int64)
    for by in range(nby):
        for bx in range(nbx):
            for tid in range(256):
                wave, lane = tid >> 6, tid & 63
                if quads:                                           # light_tiles.hpp:57-64
                    x = bx * 64 + (wave & 1) * 32 + (lane & 31)
                    y = row0 + by * 4 + (wave >> 1) * 2 + (lane >> 5)
                else:
                    x = bx * 64 + (tid & 63)
                    y = row0 + by * 4 + (tid >> 6)
                if x < w and y < row0 + rows:                       # the lanes that return at once are absent
                    want[(by * nbx + bx) * 4 + wave, lane] = y * w + x
    got = lv.wave_pixels(w, row0, rows, quads)
    assert np.array_equal(got, want)
    live = got[got >= 0]
    assert np.array_equal(np.sort(live), np.arange(row0 * w, (row0 + rows) * w))          # every pixel of the range, once


def test_kinds():
    v = np.ones((6, 64), bool); b = np.ones((6, 64), bool)
    b[1] = False
    b[2, 31] = False
    b[3] = False; b[3, 5] = True
    b[4, :20] = False
    v[5] = False
    v[2, 0] = False; b[2, 0] = False                                # a lane that does not vote does not count
    kind, lane = lv.kinds(v, b)
    assert [lv.KINDS[k] for k in kind] == ["ALL", "NONE", "ONE_OUT", "ONE_IN", "MIXED", "NO_VOTERS"]
    assert list(lane) == [-1, -1, 31, 5, -1, -1]


@pytest.fixture(scope="module")
def census():
    return lv.census()


def test_census(census):
    """Every vote a configuration can reach meets the conditions; the others are never taken.  profiles/light_votes_census.txt holds
    the counts (python tests/light_votes_lib.py writes it; test_census_file holds it to what is computed here).

    Vote 10 at lane 0: J is the first voting lane's cascade, so that lane can be the only one to refuse only by failing the magnitude
    bound while it agrees on the cascade -- a NaN position, which len_from_sq puts into cascade 0, among pixels of cascade 0 (the frame
    "first lane, vote 10")."""
    for cfg in lv.CONFIGS:
        last = 39 if cfg.chain else 7                               # the last live lane of the partial wavefront (x = 199)
        for vote in lv.VOTES:
            c = census[(cfg.name, vote)]
            k = dict(zip(lv.KINDS, c["kinds"]))
            where = (cfg.name, vote)
            if not lv.reachable(cfg, vote):
                assert sum(c["kinds"][:5]) == 0, where
                continue
            if not lv.laid_out(cfg, vote):
                continue
            assert k["ALL"] >= 4, where
            assert k["NONE"] + k["MIXED"] >= 4, where
            for lane in lv.SPOILER_LANES:
                assert c["one_out"].get(lane, 0) >= 1, (where, lane)
            assert c["one_out_partial"].get(last, 0) >= 1, where
            assert c["all_partial"] >= 1, where
            assert c["all_uncovered_spoiler"] >= 1, where
            if vote == "10":
                assert c["all_first_not_0"] >= 4, where


def test_census_file():
    """The committed table is the one the corpus gives."""
    with open(lv.CENSUS_FILE) as fh:
        assert fh.read() == lv.census_report()


def test_census_cascade_sets():
    """Votes 9, 10: wavefronts that hold exactly the cascades {0}, {0, 2}, {2, 3}, {3, 4} and all five, and wavefronts whose first
    voting lane is in cascade 3 while every other one is in 0 -- under both footprints."""
    for footprint, n in lv.cascade_set_census().items():
        for k, count in n.items():
            assert count >= 2, (footprint, k, count)


def test_census_vote_10_first_lane(census):
    """Vote 10, besides: wavefronts whose first voting lane is in another cascade than all the others (J comes from the one lane that
    disagrees: ONE_IN at the first lane)."""
    co = lv.corpus()
    for cfg in lv.CONFIGS:
        if not lv.reachable(cfg, "10"):
            continue
        idx = lv.wave_pixels(lv.W, 0, lv.H, cfg.chain)
        n = 0
        for fr in co.frames:
            fields = lv.call_fields(co, fr, cfg)
            for vote, sub, voters, bits, idle in lv.wave_votes(fields, idx, cfg.radius, cfg.flags, cfg.chain, gloss=cfg.gloss):
                if vote == "10":
                    kind, lane = lv.kinds(voters, bits)
                    full = voters.sum(1) >= 32
                    n += int(((kind == lv.KINDS.index("ONE_IN")) & (lane == voters.argmax(1)) & full).sum())
        assert n >= 4, cfg.name


def test_point_shadow_lights_reach_the_corpus(built_lib, oracle):
    """The local lights of the point-shadow configuration light pixels of every frame (its references are not the literal frame's)."""
    ps = [c for c in lv.CONFIGS if c.family == "point shadows"][0]
    for k in range(len(lv.corpus().frames)):
        assert (lv.reference(oracle, k, ps, 0, lv.H)[0] != lv.reference(oracle, k, lv.CONFIGS[0], 0, lv.H)[0]).any(), k


def test_census_quads():
    """Vote 13 (quad derivatives from covered neighbours only): quads with one, two and three covered pixels; among those with two
    and with three, quads where the derivative through a covered neighbour puts a covered pixel above level 0 (a coverage bit read
    wrongly then changes the level); with one covered pixel there is no derivative and the level is 0.  No quad is split by the end
    of a call: frame heights are even and a chain call covers whole quad rows (test_light_votes_gpu.py pins the refusals)."""
    q = lv.quad_census()
    assert (q["covered"] >= 4).all(), q
    assert q["minified"][2] >= 4 and q["minified"][3] >= 4 and q["minified"][4] >= 4, q
    assert q["minified"][0] == 0 and q["minified"][1] == 0, q


def test_census_equal_depths(hostsim):
    """Votes 2, 3, 12: reference depths exactly equal to the decoded texel under the footprint (a shortcut that compares in another
    domain -- d24_threshold -- or rounds the reference differently shows there and nowhere else), with either value of the lowest
    mantissa bit."""
    even, odd = lv.equal_depth_values(hostsim)
    assert even >= 4 and odd >= 4, (even, odd)


@pytest.mark.parametrize("cfg", lv.CONFIGS, ids=[c.name for c in lv.CONFIGS])
def test_host_bodies_equal_oracle(built_lib, oracle, hostsim, cfg):
    """The kernel bodies on the host == the oracle (the point-shadow and the general family: their checkers) on every frame of the corpus, as the whole
    frame and as the three row ranges."""
    co = lv.corpus()
    local = cfg.family == "point shadows"
    cb = lv.local_lights()["cb"] if local else co.cb
    kw = lv.light_kwargs() if local else {}
    for k, fr in enumerate(co.frames):
        p = dict(lv.planes_of(fr, cfg)[0], cube=lv.cube_of(co, cfg))
        for row0, rows in lv.ROW_RANGES:
            ref, ref_rad = lv.reference(oracle, k, cfg, row0, rows)
            got, rad = hostsim.light_frame(cb, p, fr.ambient, lv.NUM_DIR_LIGHTS, cfg.radius, cfg.flags, row0=row0, rows=rows, cube_dim=lv.CUBE_DIM, **kw)
            assert np.array_equal(got, ref), (fr.name, row0, rows, int((got != ref).sum()))
            assert fuzz_util.same_floats(rad, ref_rad), (fr.name, row0, rows)
