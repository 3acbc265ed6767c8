"""Producer passes on triangle soups, CPU tier: the kernels' own bodies (hostsim) against the oracle on every case
of raster_soup_lib, bit for bit; and the conditions the cases must meet to be worth running on the device, checked against the
oracle alone -- exact depth ties that the draw order decides (against a numpy restatement of coverage), a partition of the target
that the draw order must not show through, both classes of the live list with boxes right at the split, fans of five triangles."""
import numpy as np
import pytest

import oracle_lib
import raster_soup_lib as soup

PLANES = {1: ("depth", "normal"), 2: ("depth", "g0", "g1", "g2")}


def bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32)


def run_oracle(orc, case, mode, bias=(0, 0.0), viewproj=None, dim=None):
    W, H = (case["W"], case["H"]) if mode else ((dim or case["shadow_dim"]),) * 2
    return oracle_lib.rasterize(orc, mode, case["view"], case["viewproj"] if viewproj is None else viewproj, case["items"],
                                case["materials"], case["textures"], W, H, *bias)


def assert_no_nan(r):
    for k in ("normal", "g0", "g1", "g2"):
        if r[k] is not None:
            assert np.isfinite(r[k].astype(np.float32)).all(), k


@pytest.mark.parametrize("name", soup.CASE_NAMES)
def test_kernel_bodies_match_oracle(built_lib, oracle, hostsim, name):
    """Modes 1 and 2 and the shadow pass with and without its bias: every plane and the count of set-up triangles."""
    case = soup.get(name)
    mats = case["materials"]
    for mode, bias in ((0, (10000, 2.0)), (0, (0, 0.0)), (1, (0, 0.0)), (2, (0, 0.0))):
        a = run_oracle(oracle, case, mode, bias)
        W, H = a["depth"].shape[1], a["depth"].shape[0]
        b = hostsim.rasterize(mode, case["view"], case["viewproj"], case["items"], mats, case["textures"], W, H, *bias)
        assert a["tris"] == b["tris"], (mode, a["tris"], b["tris"])
        assert np.array_equal(a["depth"], b["depth"]), mode
        assert_no_nan(a)
        for k in PLANES.get(mode, ()):
            assert np.array_equal(bits(a[k]), bits(b[k])), (mode, k)
    assert (a["depth"] < 0xFFFFFF).any()


@pytest.mark.parametrize("name", ["stack", "stack-empties"])
def test_stack_ties_go_to_the_earliest_primitive(built_lib, oracle, name):
    """Every overlap in `stack` is an exact D24 tie.  The owner of each pixel, by a numpy restatement of coverage (exact integer
    edge functions, top-left rule) and "first in draw order", is named by the normal plane (its triangle) and by G1 (its instance)."""
    case = soup.get(name)
    W, H = case["W"], case["H"]
    counts = soup.item_counts(case["items"])
    lead = 8 if name == "stack-empties" else 0
    assert len(counts) == soup.STACK_ITEMS + lead and all(n == 0 or m == 0 for n, m in counts[:lead])
    assert counts[lead + soup.STACK_NO_INDICES] == (0, 1) and counts[lead + soup.STACK_NO_INSTANCES][1] == 0
    assert case["items"][lead + soup.STACK_NO_INSTANCES][0] is None and sum(1 for n, m in counts if n and m) == 17
    starts, bases = [it[3] for it in case["items"]], [it[4] for it in case["items"]]
    assert min(starts) > 0 and min(bases) < 0 < max(bases)
    assert len({it[1].__array_interface__["data"][0] for it in case["items"]}) == 1       # one index buffer under every item
    win, count = soup.stack_winners(case)
    nd, gb = run_oracle(oracle, case, 1), run_oracle(oracle, case, 2)
    covered = win >= 0
    assert np.array_equal(nd["depth"] < 0xFFFFFF, covered) and (nd["depth"][covered] == 0x800000).all()
    assert (count >= 2).mean() > 0.3                                   # ties all over the frame
    normal_id = np.array([p[2] for p in case["prims"]]); material = np.array([p[3] for p in case["prims"]])
    got = nd["normal"][..., :3].astype(np.float64)
    nearest = np.argmin(((got[:, :, None, :] - case["normals"][None, None]) ** 2).sum(-1), axis=-1)
    assert np.array_equal(nearest[covered], normal_id[win[covered]])
    assert np.abs(got[covered] - case["normals"][nearest[covered]]).max() < 2e-3       # and it is that normal, to fp16
    albedo = case["materials"]["DiffuseAlbedo"][:, :3]
    assert np.array_equal(gb["g1"][covered][:, :3], albedo[material[win[covered]]])
    assert np.array_equal(gb["depth"], nd["depth"])
    # reversed draw order: the ties are real, a good part of the frame changes hands
    rev = run_oracle(oracle, soup.reversed_items(case), 1)
    assert np.array_equal(rev["depth"], nd["depth"])
    changed = (bits(rev["normal"]) != bits(nd["normal"])).any(axis=-1)
    assert changed[covered].mean() >= 0.2, changed[covered].mean()
    rwin, _ = soup.stack_winners(case, order=reversed_prim_order(case))
    assert np.array_equal(changed, normal_id[rwin] != normal_id[win])


def reversed_prim_order(case):
    """Indices into case["prims"] in the draw order of the reversed item list (instances and triangles keep their order)."""
    order, k = [], 0
    for n, m in soup.item_counts(case["items"]):
        order.append(list(range(k, k + (n // 3) * m))); k += (n // 3) * m
    assert k == len(case["prims"])
    return [p for item in order[::-1] for p in item]


def test_grid_is_a_partition_whatever_the_order(built_lib, oracle):
    """`grid` tiles the target: every pixel is covered, and since no pixel centre belongs to two triangles (or to none) along a
    shared edge, the planes do not depend on the draw order."""
    case = soup.get("grid")
    a = run_oracle(oracle, case, 1)
    assert (a["depth"] == 0x800000).all() and a["tris"] == case["triangles"]
    assert len(np.unique(bits(a["normal"]).reshape(-1, 4), axis=0)) > 0.9 * case["triangles"]
    for seed in (1, 2):
        b = run_oracle(oracle, soup.permuted(case, seed), 1)
        assert np.array_equal(a["depth"], b["depth"]) and np.array_equal(bits(a["normal"]), bits(b["normal"]))
    # the numpy restatement of coverage agrees: exactly one triangle per pixel centre
    v = case["items"][0][0]
    X, Y = soup.snap(v["Pos"].reshape(-1, 3, 3), case["W"], case["H"])
    hits = sum(soup.covers(x, y, case["W"], case["H"]).astype(np.int64) for x, y in zip(X, Y))
    assert (hits == 1).all()


def test_threshold_populates_both_classes(built_lib, oracle):
    """Boxes of 2047, 2048, 2049, 2050 and 2080 pixels; large boxes whose sides are no multiples of the 16 x 4 footprint."""
    every = []
    for variant in soup.THRESHOLD:
        case = soup.get("threshold-" + variant)
        areas = case["box_areas"]
        assert (areas > soup.LARGE_BOX).sum() >= 3 and ((areas > 0) & (areas <= soup.LARGE_BOX)).sum() >= 3, variant
        assert (areas == 2048).any(), variant
        every += list(areas)
        r = run_oracle(oracle, case, 1)
        assert r["tris"] == len(areas) and len(np.unique(r["depth"])) > 100        # all front-facing; steep depth
    assert {2047, 2048, 2049, 2050, 2080} <= set(every)


def test_clip_reaches_fans_of_five(built_lib, oracle):
    """The two heptagons of `clip`, drawn alone (in both windings: one is culled), set up five fan triangles each; the whole case
    sets up more triangles than it has front-facing inputs, and draws through the near plane down to the bottom row."""
    case = soup.get("clip")
    for name, alone in case["fans"].items():
        assert run_oracle(oracle, alone, 1)["tris"] >= 5, name
    r = run_oracle(oracle, case, 2)
    assert r["tris"] > soup.input_triangles(case["items"]) // 2
    assert (r["depth"][-1] < 0xFFFFFF).all()
    textured = r["g1"][..., 3] == case["materials"]["Roughness"][4]
    assert textured.sum() > 50 and len(np.unique(r["g1"][textured][:, 0])) > 20     # the mipped texture shows


def test_draw_item_locations_matter(built_lib, oracle):
    """The two locations are really used: with either one zeroed in every item that sets it, the oracle refuses the list (an index
    leaves its vertex buffer) or renders another image."""
    case = soup.get("mixed-0")
    ref = run_oracle(oracle, case, 1)
    for field in (3, 4):
        assert sum(1 for it in case["items"] if it[0] is not None and it[field]) >= 3
        items = [tuple(0 if k == field else x for k, x in enumerate(it)) if it[0] is not None and it[field] else it for it in case["items"]]
        try:
            got = oracle_lib.rasterize(oracle, 1, case["view"], case["viewproj"], items, case["materials"], case["textures"], case["W"], case["H"])
            outcome = "another image" if not np.array_equal(bits(got["normal"]), bits(ref["normal"])) else "the same image"
        except RuntimeError:
            outcome = "refused"
        assert outcome in ("another image", "refused"), (field, outcome)
