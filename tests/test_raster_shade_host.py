"""The shader half of the producer passes, CPU tier: hand-derived known answers for World, TexTransform and
MatTransform, asserted on the oracle and on the kernels' own bodies (hostsim); the conditions the cases of raster_shade_lib must meet
to be worth running on the device, checked against the oracle alone; and the kernel bodies against the oracle, bit for bit, on
every case.  The known answers use neither the oracle's nor the kernels' helpers nor the case library's matrix builders: every matrix
below is written out, in the row-vector convention of the shaders (v' = v . M) and stored transposed by T()."""
import numpy as np
import pytest

import oracle_lib
import raster_shade_lib as shade
from oracle_lib import INSTANCE_DT, MATERIAL_DT, VERTEX_DT

PLANES = {1: ("depth", "normal"), 2: ("depth", "g0", "g1", "g2")}
EYE4 = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]


def bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32)


def T(m):
    """A matrix written row by row as the 16 floats a record stores: its transpose, flattened."""
    return np.array(m, np.float32).T.reshape(16).copy()


def both(oracle, hostsim):
    """The two implementations under the same call: (name, f(mode, view, viewproj, items, materials, textures, W, H))."""
    return (("oracle", lambda *a: oracle_lib.rasterize(oracle, *a)), ("kernel bodies", lambda *a: hostsim.rasterize(*a)))


def one_instance(world=EYE4, tex=EYE4, material=0):
    inst = np.zeros(1, INSTANCE_DT)
    inst["World"] = T(world); inst["TexTransform"] = T(tex); inst["MaterialIndex"] = material
    return inst


def one_material(mat=EYE4, dmap=0, nmap=9):
    m = np.zeros(1, MATERIAL_DT)
    m["DiffuseAlbedo"] = 1.0; m["Roughness"] = 0.25; m["Metalness"] = 0.75
    m["MatTransform"] = T(mat); m["DiffuseMapIndex"] = dmap; m["NormalMapIndex"] = nmap
    return m


def full_frame_quad():
    """The whole target at z = 0.5 under identity View / ViewProj: TexC (0, 0) at the top-left pixel corner, (1, 1) at the bottom-right."""
    v = np.zeros(4, VERTEX_DT)
    v["Pos"] = [(-1, 1, 0.5), (1, 1, 0.5), (1, -1, 0.5), (-1, -1, 0.5)]
    v["TexC"] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    v["Normal"] = (0, 0, -1); v["TangentU"] = (1, 0, 0)
    return v, np.array([0, 1, 2, 0, 2, 3], np.uint32)


def coordinate_level0(size=32):
    """Texel (x, y) = (8 x, 8 y, 77, 255), a single level: a sample at a texel centre is that texel."""
    y, x = np.mgrid[0:size, 0:size]
    return np.stack([8 * x, 8 * y, np.full_like(x, 77), np.full_like(x, 255)], axis=-1).astype(np.uint8)


def textured_frame(run, W, H, tex, mat):
    v, idx = full_frame_quad()
    r = run(2, T(EYE4), T(EYE4), [(v, idx, one_instance(tex=tex))], one_material(mat), [coordinate_level0()], W, H)
    assert (r["depth"] == 0x800000).all()
    return r["g1"][..., :2].astype(np.float64) * 255.0          # (8 x texel, 8 y texel) as sampled


# ---- known answers ----------------------------------------------------------------------------------------------------------
# XMMatrixRotationX / Y / Z (+-90 degrees), written out; (1, 0, 0) . M is the first row
QUARTER = {
    "x+": ([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], (1, 0, 0)),
    "x-": ([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], (1, 0, 0)),
    "y+": ([[0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]], (0, 0, -1)),
    "y-": ([[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1]], (0, 0, 1)),
    "z+": ([[0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], (0, 1, 0)),
    "z-": ([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], (0, -1, 0)),
}
# a View whose 3 x 3 has nine different entries, all exact in binary16; only its 3 x 3 reaches a pixel (DrawNormals.hlsl:91)
VIEW = [[0.25, -0.5, 0.75, 0], [0.125, 0.875, -0.375, 0], [-0.625, 0.0625, 0.3125, 0], [0, 0, 0, 1]]


@pytest.mark.parametrize("turn", list(QUARTER))
def test_quarter_turns_permute_the_normal(built_lib, oracle, hostsim, turn):
    """A flat face with normal +x under an exact quarter turn: NormalW = (1, 0, 0) . World is the first row of World, G2 holds exactly
    that axis, and the half4 normal of mode 1 is that axis through View: +- a row of View's 3 x 3.  The positions are chosen so that
    the turned triangle faces the camera: Pos = Q . World^T for a fixed clockwise triangle Q."""
    world, axis = QUARTER[turn]
    w3 = np.array(world, np.float64)[:3, :3]
    q = np.array([(-0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0.0, -0.5, 0.5)])
    v = np.zeros(3, VERTEX_DT)
    v["Pos"] = q @ w3.T
    v["Normal"] = (1, 0, 0); v["TangentU"] = (0, 1, 0)
    assert np.array_equal(v["Pos"].astype(np.float64) @ w3, q)
    items = [(v, np.array([0, 1, 2], np.uint32), one_instance(world=world))]
    k = int(np.argmax(np.abs(axis)))
    expect_view = (np.float32(axis[k]) * np.array(VIEW, np.float32)[k, :3]).astype(np.float16)
    for who, run in both(oracle, hostsim):
        g = run(2, T(VIEW), T(EYE4), items, one_material(dmap=9), None, 40, 24)
        cov = g["depth"] < 0xFFFFFF
        assert cov.sum() > 100, who
        assert (g["g2"][cov] == np.array(axis + (1.0,), np.float32)).all(), (who, turn)
        n = run(1, T(VIEW), T(EYE4), items, one_material(dmap=9), None, 40, 24)
        assert np.array_equal(n["depth"], g["depth"])
        assert (bits(n["normal"][cov][:, :3]) == bits(expect_view)).all(), (who, turn)


def test_tex_transform_translation_shifts_by_whole_texels(built_lib, oracle, hostsim):
    """32 x 32 pixels over a 32 x 32 texture: pixel (x, y) samples texel (x, y) at its centre.  TexTransform = translation
    (0.25, 0.5) moves that to texel ((x + 8) mod 32, (y + 16) mod 32)."""
    shift = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.25, 0.5, 0, 1]]
    y, x = np.mgrid[0:32, 0:32]
    for who, run in both(oracle, hostsim):
        plain, moved = textured_frame(run, 32, 32, EYE4, EYE4), textured_frame(run, 32, 32, shift, EYE4)
        assert np.abs(plain - np.stack([8 * x, 8 * y], axis=-1)).max() < 1e-3, who
        assert np.abs(moved - np.stack([8 * ((x + 8) % 32), 8 * ((y + 16) % 32)], axis=-1)).max() < 1e-3, who


def test_reference_scaling_repeats_the_pattern_eight_times(built_lib, oracle, hostsim):
    """XMMatrixScaling(8, 8, 1), the reference's own TexTransform, over 64 x 64 pixels: u = (x + 1/2) / 8, so pixel x samples at
    texel 4 (x mod 8) + 1.5 -- half way between two texels, value 8 (4 (x mod 8) + 1.5) -- and the pattern repeats every 8 pixels,
    eight times across the quad."""
    scale = [[8, 0, 0, 0], [0, 8, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    y, x = np.mgrid[0:64, 0:64]
    for who, run in both(oracle, hostsim):
        got = textured_frame(run, 64, 64, scale, EYE4)
        assert np.abs(got - np.stack([32 * (x % 8) + 12, 32 * (y % 8) + 12], axis=-1)).max() < 1e-3, who
        assert np.abs(got[:, 8:] - got[:, :-8]).max() < 1e-3 and np.abs(got[:, 4:, 0] - got[:, :-4, 0]).min() > 100, who


def test_scale_then_translate_is_not_translate_then_scale(built_lib, oracle, hostsim):
    """TexC . TexTransform . MatTransform over 64 x 32 pixels (u = (x + 1/2) / 64).  Scale (2, 1) in the instance and translate
    (0.25, 0) in the material: u' = 2 u + 0.25, texel x + 8.  The reverse: u' = 2 (u + 0.25), texel x + 16.  Eight texels apart."""
    scale = [[2, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    shift = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.25, 0, 0, 1]]
    y, x = np.mgrid[0:32, 0:64]
    for who, run in both(oracle, hostsim):
        a, b = textured_frame(run, 64, 32, scale, shift), textured_frame(run, 64, 32, shift, scale)
        assert np.abs(a - np.stack([8 * ((x + 8) % 32), 8 * y], axis=-1)).max() < 1e-3, who
        assert np.abs(b - np.stack([8 * ((x + 16) % 32), 8 * y], axis=-1)).max() < 1e-3, who


def test_z_and_w_columns_do_not_reach_texc(built_lib, oracle, hostsim):
    """Only .xy of the last product is kept (GeometryPass.hlsl:40).  Entries in the z and w columns of the matrix applied last --
    MatTransform, or TexTransform where the material index lies outside the buffer -- change no plane.  (In a TexTransform that a
    MatTransform follows they do count: the HLSL multiplies the whole float4 on.)"""
    xy = [[1.5, 0.25, 0, 0], [-0.5, 1.25, 0, 0], [0, 0, 1, 0], [0.375, 0.125, 0, 1]]
    zw = [[1.5, 0.25, 0.7, -0.4], [-0.5, 1.25, -1.3, 0.6], [0, 0, 0.9, 0.2], [0.375, 0.125, 0.5, 0.35]]
    v, idx = full_frame_quad()
    for who, run in both(oracle, hostsim):
        for tex_a, tex_b, mat_a, mat_b, index in ((EYE4, EYE4, xy, zw, 0), (xy, zw, EYE4, EYE4, 5)):
            a = run(2, T(EYE4), T(EYE4), [(v, idx, one_instance(tex=tex_a, material=index))], one_material(mat_a), [coordinate_level0()], 48, 40)
            b = run(2, T(EYE4), T(EYE4), [(v, idx, one_instance(tex=tex_b, material=index))], one_material(mat_b), [coordinate_level0()], 48, 40)
            assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in PLANES[2]), (who, index)
            assert len(np.unique(a["g1"][..., 0])) > 20, who


# ---- the cases' conditions, against the oracle alone ------------------------------------------------------------------------
def run_oracle(orc, case, mode, bias=(0, 0.0)):
    W, H = (case["W"], case["H"]) if mode else (case["shadow_dim"],) * 2
    return oracle_lib.rasterize(orc, mode, case["view"], case["viewproj"], case["items"], case["materials"], case["textures"], W, H, *bias)


@pytest.mark.parametrize("name", shade.CASE_NAMES)
def test_cases_cover_a_fifth_of_their_frame(built_lib, oracle, name):
    case = shade.get(name)
    assert case["W"] * case["H"] <= 130 * 70 and case["shadow_dim"] <= 64
    assert (run_oracle(oracle, case, 1)["depth"] < 0xFFFFFF).mean() >= 0.2
    assert (run_oracle(oracle, case, 0)["depth"] < 0xFFFFFF).mean() >= 0.2


def test_world_mirror_flips_the_culling(built_lib, oracle):
    """The mirrored instance draws the faces its unmirrored twin culls, and the reverse: of the twin the whole front sheet and
    nothing of the back sheet is set up, of the mirror nothing of the front sheet and the whole back sheet.  Every instance shows."""
    case = shade.get("world")
    tris = {k: run_oracle(oracle, p, 1)["tris"] for k, p in case["probes"].items()}
    n = len(case["probes"][("twin", "front")]["items"][0][0]) // 3
    assert tris == {("twin", "front"): n, ("twin", "back"): 0, ("mirror", "front"): 0, ("mirror", "back"): n}, tris
    g = run_oracle(oracle, case, 2)
    cov = g["depth"] < 0xFFFFFF
    shown = [int((cov & (g["g1"][..., 3] == r)).sum()) for r in case["materials"]["Roughness"]]
    assert min(shown) >= 30, shown
    assert len(case["items"]) == 1 and case["items"][0][2] is not None and len(case["items"][0][2]) * (len(case["items"][0][1]) - case["items"][0][3]) // 3 > 128


def test_texc_outside_material_reads_the_defaults(built_lib, oracle):
    case = shade.get("texc")
    inst = case["items"][0][2]
    assert (inst["MaterialIndex"] >= len(case["materials"])).sum() == 1
    g = run_oracle(oracle, case, 2)
    cov = g["depth"] < 0xFFFFFF
    default = cov & (g["g1"][..., 3] == 0.5)
    assert default.sum() > 100 and (g["g0"][..., 3][default] == 0.5).all()
    assert not (g["g0"][..., 3][cov & ~default] == 0.5).any()
    listed = set(case["materials"]["Roughness"].tolist())
    assert set(np.unique(g["g1"][..., 3][cov & ~default]).tolist()) == listed       # and every other instance shows its own material


def test_sampler_reaches_every_probe_count_and_level(built_lib, oracle):
    """On a copy of `sampler` whose chains are grey per level (level k = 20 (k + 1)), G1 names the level of detail of the diffuse
    lookup: lod = 255 G1 / 20 - 1.  Every stored level of every chain gets at least half the weight of some pixel (with the
    materials as they are, or with their two map indices exchanged).  Probe counts: on the ground strips TexC is the world position
    (G0) times the strip's scale, so the footprint |major| follows from G0 by the same quad differences; |major| / 2^lod is then
    the number of probes the sampler took, and wherever it agrees with clamp(ceil(|major| / |minor|), 1, 8) it counts: all of
    2 ... 8 occur.  One probe needs |major| == |minor| exactly, which no perspective footprint delivers; it is what the definition
    makes of a footprint of zero (both lengths clamp to 2^-50, ceil(1) = 1), so the quad with constant TexC takes it -- unobservably,
    since any number of probes would read the same place.  The test asserts that quad is drawn."""
    case = shade.get("sampler")
    H, W = case["H"], case["W"]
    reached = {t: set() for t in range(len(shade.SAMPLER_CHAINS))}
    probes = set()
    for swap in (False, True):
        grey = shade.with_grey_levels(case, swap)
        g = run_oracle(oracle, grey, 2)
        cov = g["depth"] < 0xFFFFFF
        lod = g["g1"][..., 0].astype(np.float64) * 255.0 / 20.0 - 1.0
        for m, mat in enumerate(grey["materials"]):
            t = int(mat["DiffuseMapIndex"])
            if t >= len(shade.SAMPLER_CHAINS):
                continue
            px = cov & (g["g1"][..., 3] == mat["Roughness"])
            levels = len(grey["textures"][t])
            assert px.any() and (lod[px] > -1e-4).all() and (lod[px] < levels - 1 + 1e-4).all()
            reached[t] |= {k for k in range(levels) if (np.abs(lod[px] - k) <= 0.5).any()}
            # the ground strip of material m: whole 2 x 2 quads of its pixels in the lower half of the frame
            quad = px[0::2, 0::2] & px[1::2, 0::2] & px[0::2, 1::2] & px[1::2, 1::2]
            quad[: H // 4 + 1] = False
            if not quad.any():
                continue
            tw, th = shade.SAMPLER_CHAINS[t][:2]
            uv = g["g0"][..., [0, 2]].astype(np.float64) * case["ground_scale"][m] * [tw, th]      # in level-0 texels
            ddx = (uv[0::2, 1::2] - uv[0::2, 0::2])[quad]; ddy = (uv[1::2, 0::2] - uv[0::2, 0::2])[quad]
            lx, ly = np.hypot(ddx[:, 0], ddx[:, 1]), np.hypot(ddy[:, 0], ddy[:, 1])
            pmax, pmin = np.maximum(lx, ly), np.minimum(lx, ly)
            expect = np.clip(np.ceil(pmax / pmin), 1, 8)
            q_lod = lod[0::2, 0::2][quad]
            free = (q_lod > 0.01) & (q_lod < levels - 1 - 0.01)                      # not clamped: the level of detail is log2(|major| / N)
            took = pmax / 2.0 ** q_lod
            agree = free & (np.abs(took - expect) < 0.05 * expect)
            probes |= set(expect[agree].astype(int).tolist())
    assert reached == {t: set(range(len(case["textures"][t]))) for t in reached}, reached
    assert probes == set(range(2, 9)), probes
    constant = 0
    for v, idx, inst, start, base in case["items"]:
        tri = v["TexC"][idx[start:].astype(np.int64) + base].reshape(-1, 3, 2)
        constant += int(((tri == tri[:, :1]).all(axis=(1, 2)) & (len(inst) > 0)).sum())
    assert constant == 2


def test_sampler_pairs_every_mipped_combination(built_lib):
    """resolve_pixel's `mipped`: diffuse mipped with a plain normal map, the reverse, both mipped with different sizes; a null entry
    and an index outside the table on either side; every entry of the table used."""
    case = shade.get("sampler")
    tex = case["textures"]
    kind = lambda i: "outside" if i >= len(tex) else "null" if tex[i] is None else "mipped" if isinstance(tex[i], list) else "plain"
    pairs = {(kind(int(m["DiffuseMapIndex"])), kind(int(m["NormalMapIndex"]))) for m in case["materials"]}
    assert {("mipped", "plain"), ("plain", "mipped"), ("mipped", "mipped"), ("mipped", "null"), ("outside", "mipped")} <= pairs
    used = set(case["materials"]["DiffuseMapIndex"].tolist()) | set(case["materials"]["NormalMapIndex"].tolist())
    assert used >= set(range(len(tex)))
    assert [len(t) for t in tex[:5]] == [5, 3, 5, 5, 3] and tex[0][0].shape == (10, 24, 4) and tex[2][0].shape == (16, 1, 4)
    both_mipped = [(tex[int(m["DiffuseMapIndex"])][0].shape, tex[int(m["NormalMapIndex"])][0].shape) for m in case["materials"]
                   if kind(int(m["DiffuseMapIndex"])) == kind(int(m["NormalMapIndex"])) == "mipped"]
    assert any(a != b for a, b in both_mipped)


def test_nonfinite_texc_reaches_the_pixels(built_lib, oracle):
    """The three non-finite coordinates really arrive at pixels (they change G1 against a finite stand-in) and leave every plane finite."""
    case = shade.get("nonfinite")
    g = run_oracle(oracle, case, 2)
    for k in ("g0", "g1", "g2"):
        assert np.isfinite(g[k]).all(), k
    items = []
    for it in case["items"]:
        v = it[0].copy()
        v["TexC"] = np.nan_to_num(it[0]["TexC"], nan=0.5, posinf=0.5, neginf=0.5)
        items.append((v,) + tuple(it[1:]))
    assert (~np.isfinite(case["items"][0][0]["TexC"])).any(axis=1).sum() >= 3          # one vertex buffer under all three items
    h = run_oracle(oracle, dict(case, items=items), 2)
    changed = (bits(h["g1"]) != bits(g["g1"])).any(-1)
    for r in np.unique(g["g1"][..., 3][g["depth"] < 0xFFFFFF]):
        assert changed[g["g1"][..., 3] == r].mean() > 0.2, r


# ---- the kernel bodies against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", shade.CASE_NAMES)
def test_kernel_bodies_match_oracle(built_lib, oracle, hostsim, name):
    """Modes 1 and 2 and the shadow pass with and without its bias: every plane, bit for bit, and the count of set-up triangles.
    Every plane is finite, those of `nonfinite` (NaN, +inf and -inf TexC) and `tbn` (zero and parallel tangents) included."""
    case = shade.get(name)
    for mode, bias in ((0, (10000, 2.0)), (0, (0, 0.0)), (1, (0, 0.0)), (2, (0, 0.0))):
        a = run_oracle(oracle, case, mode, bias)
        H, W = a["depth"].shape
        b = hostsim.rasterize(mode, case["view"], case["viewproj"], case["items"], case["materials"], case["textures"], W, H, *bias)
        assert a["tris"] == b["tris"], (mode, a["tris"], b["tris"])
        assert np.array_equal(a["depth"], b["depth"]), mode
        for k in PLANES.get(mode, ())[1:]:
            assert np.isfinite(a[k].astype(np.float32)).all() and np.isfinite(b[k].astype(np.float32)).all(), (mode, k)
            assert np.array_equal(bits(a[k]), bits(b[k])), (mode, k)
