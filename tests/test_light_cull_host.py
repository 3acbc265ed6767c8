"""The tiled cull of the local lights (csrc/light_tiles.hpp light_local_tile) on the host.  tests/hostsim's tiled mode culls per 64 x 4
tile with the very functions the kernels call (light_core.hpp tile_box_pixel / tile_box_merge / tile_box_any_covered /
tile_light_touches) and walks each tile's admitted lights only; the statement is

    un-culled host body == tiled host body == frozen checker      (RGBA8 bit-equal, radiance equal up to NaN payloads)

on fuzz frames with thinned non-finite world positions and 1024 + 1024 lights (fuzz_util.light_cull_case), for every local kernel
family, whole frames and row ranges; on light counts around the mask words and the 256-stride of the cull loop; and on hand-built
one-tile frames at the edges of the sphere-against-box test.  Each case set first asserts, from the tiled host's masks, that its
inputs do exercise the cull (share of admitted lights, every mask word, tiles where a non-finite pixel meets a light the finite
pixels' box rejects)."""
import numpy as np
import pytest

import fuzz_util
import light_cull_cases as lc


def _same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), (what, int((got[0] != ref[0]).any(-1).sum()))
    assert fuzz_util.same_floats(got[1], ref[1]), what


def _finite_only_masks(case, hostsim):
    """The masks of the frame with every covered non-finite position taken out of the coverage: what the finite pixels' box alone
    admits."""
    depth = case.planes["depth"].copy()
    depth[case.covered() & ~case.finite()] |= 0xFFFFFF
    planes, case.planes = case.planes, dict(case.planes, depth=depth)
    try:
        return lc.mask_bits(case.host(hostsim, True)[2])
    finally:
        case.planes = planes


class _Conditions:
    """What a case set has to show before its comparisons count.  The bounds were fixed before the generator was shaped to meet them
    and say that the cull both bites and is at risk: 10 % .. 50 % of the non-empty tiles hold a non-finite covered position; over
    the tiles of finite positions 0.02 .. 0.6 of the (tile, light) pairs are admitted; each of the 32 words of each mask is
    non-zero in some tile and not all-ones in some tile; at least 20 tiles hold a non-finite pixel together with a light that the
    finite pixels' box alone rejects.  They are conditions on the inputs, not measurements of the code."""

    def __init__(self):
        self.tiles = self.dirty = self.defect = 0
        self.pairs = self.admitted = 0
        self.some, self.not_all = None, None

    def add(self, case, bits, finite_bits):
        cov, fin = case.covered(), case.finite()
        lists = [k for k, n in enumerate((len(case.point_records), len(case.spot_records))) if n == 1024]
        if self.some is None:
            self.some = np.zeros((2, 32), bool)
            self.not_all = np.zeros((2, 32), bool)
            self.lists = lists
        for ty in range(bits.shape[0]):
            for tx in range(bits.shape[1]):
                c, f = lc.tile_view(cov, ty, tx), lc.tile_view(fin, ty, tx)
                if not c.any():
                    assert not bits[ty, tx].any()                      # an empty tile admits nothing
                    continue
                self.tiles += 1
                words = np.packbits(bits[ty, tx], axis=-1, bitorder="little").view(np.uint32)
                self.some |= words != 0
                self.not_all |= words != 0xFFFFFFFF
                if (c & ~f).any():
                    self.dirty += 1
                    self.defect += bool((~finite_bits[ty, tx][lists]).any())
                else:
                    self.pairs += 1024 * len(lists)
                    self.admitted += int(bits[ty, tx][lists].sum())

    def check(self):
        share_dirty, share_admitted = self.dirty / self.tiles, self.admitted / self.pairs
        print("tiles %d, with a non-finite position %d (%.3f), admitted share over finite tiles %.3f, defect tiles %d" %
              (self.tiles, self.dirty, share_dirty, share_admitted, self.defect))
        assert 0.10 <= share_dirty <= 0.50, share_dirty
        assert 0.02 <= share_admitted <= 0.6, share_admitted
        assert self.some[self.lists].all() and self.not_all[self.lists].all()
        assert self.defect >= 20, self.defect


@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_fuzz_frames_culled_equals_unculled_equals_checker(built_lib, hostsim, family):
    """The family's case set (a coherent and an incoherent frame): the input conditions, then the three-way equality on the whole
    frame, then the tiled body over the three row ranges (the last anchored off the tile grid, the last tile row 2 rows high)."""
    cond = _Conditions()
    frames = []
    for seed in lc.seeds_of(family):
        case = lc.Case(family, seed, built_lib)
        cov, fin = case.covered(), case.finite()
        out, rad, masks = case.host(hostsim, True)
        bits = lc.mask_bits(masks)
        cond.add(case, bits, _finite_only_masks(case, hostsim))
        # the frame has what the generator promises: a tile whose covered positions are all NaN, tiles with exactly one non-finite one
        per_tile = [(lc.tile_view(cov, ty, tx), lc.tile_view(cov & ~fin, ty, tx), lc.tile_view(np.isnan(case.wide["g0"][..., :3]).any(-1), ty, tx))
                    for ty in range(bits.shape[0]) for tx in range(bits.shape[1])]
        assert any(c.any() and (n[c]).all() for c, _, n in per_tile)
        assert sum(int(d.sum()) == 1 for _, d, _ in per_tile) >= 2
        frames.append((case, (out, rad)))
    cond.check()
    for case, tiled in frames:
        ref = case.reference()
        _same(case.host(hostsim, False), ref, (family, case.seed, "un-culled"))
        _same(tiled, ref, (family, case.seed, "tiled"))
        out, rad = np.zeros_like(ref[0]), np.zeros_like(ref[1])
        for r0, rn in fuzz_util.CULL_ROW_RANGES:
            o, r, m = case.host(hostsim, True, row0=r0, rows=rn)
            assert m.shape[:2] == ((rn + 3) // 4, 3)
            out[r0:r0 + rn], rad[r0:r0 + rn] = o[r0:r0 + rn], r[r0:r0 + rn]
        _same((out, rad), ref, (family, case.seed, "row ranges"))


def count_case(family, n, built_lib):
    """A coherent frame of finite positions and n lights per list of which only the last is in range of tile (1, 8): the others
    sit far outside the frame's positions with a short range.  Returns (case, (tile y, tile x))."""
    ty, tx = 8, 1
    case = lc.Case(family, 100, built_lib, n, n)
    g0 = case.planes["g0"].copy()
    bad = ~np.isfinite(g0[..., :3]).all(-1)
    g0[bad, :3] = g0[~bad][0, :3]                             # a finite position of the same plane
    centre = lc.tile_view(g0, ty, tx)[2, 32, :3]

    def lights(rec):
        rec = rec.copy()
        rec["Position"] = (np.array([900.0, 900.0, 900.0]) + np.arange(len(rec))[:, None]).astype(np.float32)
        rec["FalloffEnd"], rec["FalloffStart"] = 4.0, 1.0
        if len(rec):
            rec["Position"][-1] = centre + np.float32([0.0, 0.25, 0.0])
            rec["FalloffEnd"][-1] = 0.5
            rec["Strength"][-1] = 2.4
            rec["SpotPower"][-1] = 0.0
        return rec
    case = lc.Case(family, 100, built_lib, n, n, lights=(lights(case.point_records), lights(case.spot_records)))
    case.planes = dict(case.planes, g0=g0)
    case.wide = dict(case.wide, g0=g0)
    return case, (ty, tx)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 1023])
def test_light_counts_last_light_alone_in_range(built_lib, hostsim, n):
    """n point and n spot lights, the last of each list the only one in range of one tile: that tile's masks hold bit n - 1 alone
    (mask words 0, 1, 7, 8 and 31, both trips of the cull loop's stride of 256), every tile's masks are within the count, the light
    shows in the frame, and un-culled == tiled == checker."""
    case, (ty, tx) = count_case("points_spots", n, built_lib)
    out, rad, masks = case.host(hostsim, True)
    bits = lc.mask_bits(masks)
    assert not bits[..., n:].any()
    want = np.zeros(1024, bool); want[n - 1] = True
    assert np.array_equal(bits[ty, tx, 0], want) and np.array_equal(bits[ty, tx, 1], want)
    ref = case.reference()
    _same(case.host(hostsim, False), ref, (n, "un-culled"))
    _same((out, rad), ref, (n, "tiled"))
    none = lc.Case("points_spots", 100, built_lib, 0, 0)
    none.planes, none.wide = case.planes, case.wide
    dark = none.host(hostsim, False)
    lit = lc.tile_view(rad != dark[1], ty, tx).any()
    assert lit, "the last light does not reach its tile"


def test_direct_cases_on_one_tile(built_lib, hostsim):
    """A 4 x 2 frame -- one tile -- with two covered pixels at (1, 2, 3) and (11, 12, 13) and hand-placed lights, as point lights and
    as spot lights: the masks are what the sphere-against-box test says, and un-culled == tiled == checker.
      0  at distance exactly FalloffEnd from a pixel (on the x axis: the distances are exact)          admitted
      1  inside the inflation (FalloffEnd * 1.0001 + 1e-3) but beyond FalloffEnd                     admitted, adds nothing
      2  just beyond the inflation                                                                  rejected
      3  inside the box, out of range of both pixels                                                admitted, adds nothing
      4  at a pixel's position (d = 0: the term is NaN)                                             admitted
      5  far away with FalloffEnd at the largest finite float                                       admitted
      6  far away with FalloffEnd NaN                                                               admitted
      7  a NaN Position component, out of range on the other axes                                   admitted
      8  an infinite Position component, finite FalloffEnd                                          rejected
      9  an infinite Position component, infinite FalloffEnd                                        admitted"""
    import oracle_lib
    import point_shadow_lib
    W, H = 4, 2
    _, _, planes, c, knobs = fuzz_util.random_case(3, built_lib, size=(W, H))
    depth = np.full((H, W), 0xFFFFFF, np.uint32)
    depth[0, 1] = depth[1, 2] = 0x800000
    g0 = planes["g0"].copy()
    g0[..., :3] = 7.0
    g0[0, 1, :3], g0[1, 2, :3] = (1.0, 2.0, 3.0), (11.0, 12.0, 13.0)
    fmax = float(np.finfo(np.float32).max)
    spec = [((-3.0, 2.0, 3.0), 4.0, True), ((-3.001, 2.0, 3.0), 4.0, True), ((-3.01, 2.0, 3.0), 4.0, False), ((6.0, 7.0, 8.0), 0.5, True),
            ((11.0, 12.0, 13.0), 4.0, True), ((500.0, -400.0, 300.0), fmax, True), ((500.0, -400.0, 300.0), np.nan, True),
            ((np.nan, 500.0, 3.0), 1.0, True), ((np.inf, 2.0, 3.0), 4.0, False), ((-np.inf, 2.0, 3.0), np.inf, True)]
    rec = np.zeros(len(spec), fuzz_util.LIGHT_DT)
    rec["Strength"], rec["FalloffStart"], rec["SpotPower"] = 1.0, 1.0, 8.0
    rec["Direction"] = (0.3, -2.0, 0.5)
    for k, (pos, end, _) in enumerate(spec):
        rec["Position"][k], rec["FalloffEnd"][k] = pos, end
    p = {"g0": g0, "g1": planes["g1"], "g2": planes["g2"], "depth": depth, "shadow": planes["shadow"], "cube": planes["cube"]}
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    want = np.zeros(1024, bool); want[:len(spec)] = [a for _, _, a in spec]
    for lists in (("points",), ("spots",), ("points", "spots")):
        kw = {k: fuzz_util.lights_from_records(rec) for k in lists}
        out, rad, masks = hostsim.light_frame_tiled(c.pass_cb, p, None, 3, 0.0, 1, **kw)
        bits = lc.mask_bits(masks)
        assert bits.shape[:2] == (1, 1)
        for k, name in enumerate(("points", "spots")):
            assert np.array_equal(bits[0, 0, k], want if name in lists else np.zeros(1024, bool)), (lists, name, bits[0, 0, k][:len(spec)])
        ref = point_shadow_lib.load().checker(pcb, p, None, 3, 0.0, 1, **kw)
        _same(hostsim.light_frame(c.pass_cb, p, None, 3, 0.0, 1, **kw), ref, (lists, "un-culled"))
        _same((out, rad), ref, (lists, "tiled"))
