"""The shader half of the producer passes, device tier: the HIP rasteriser through the C ABI against the oracle, bit
for bit on every plane, on the cases of raster_shade_lib -- World with a real 3 x 3 (rotations, shear, mirror), TexTransform and
MatTransform that do not commute, mip chains that are not square powers of two, saturated normal maps with degenerate tangents, and
non-finite TexC.  Only this tier meets the amdgcn lowering of resolve_pixel's fp64 interpolation, of the `%` wrap on sizes that are no
power of two and of the float -> int conversions on these inputs.  test_raster_shade_host.py shows the cases meet their conditions and
pins them by known answers; test_raster_restatement.py holds the oracle to the HLSL.  Every test here wants crychic_raster_status == 0."""
import numpy as np
import pytest

import gbuffer_f16_lib as gf
import raster_shade_lib as shade
from test_raster_soup_gpu import (BIASES, DEPTH_POISON, G_POISON, bits, check_planes, ctx, geometry, pass_cb,  # noqa: F401
                                  reference, run_pass, status)

torch = pytest.importorskip("torch")


def finite(plane_bits):
    """Whether a plane given as raw uint16 (half) or uint32 (float) bit patterns holds finite numbers only."""
    return bool(np.isfinite(plane_bits.view(np.float16 if plane_bits.dtype == np.uint16 else np.float32).astype(np.float32)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", shade.CASE_NAMES)
def test_every_pass_matches_the_oracle(ctx, built_lib, oracle, name):
    """Normals + depth, the G-buffer, the fused pass and the shadow pass with and without its bias; each issued twice into poisoned
    targets: equal to each other and to the oracle, and finite on both sides (`nonfinite` included: NaN and infinite TexC address
    texels, they do not spread)."""
    case = shade.get(name)
    geo, cb, W, H = geometry(ctx, case), pass_cb(built_lib, case), case["W"], case["H"]
    nd, gb = reference(oracle, case, 1), reference(oracle, case, 2)             # reference() asserts the oracle's planes finite
    assert np.array_equal(nd["depth"], gb["depth"])
    for which in ("normals", "gbuffer", "fused"):
        first, second = (run_pass(ctx, built_lib, geo, cb, which, W, H) for _ in range(2))
        assert all(np.array_equal(first[k], second[k]) for k in first), which
        check_planes(first, nd, gb, which)
        assert all(finite(v) for k, v in first.items() if k != "depth"), which
    dim = case["shadow_dim"]
    for bias in BIASES:
        ref = reference(oracle, case, 0, bias)
        maps = []
        for _ in range(2):
            m = torch.full((dim, dim), DEPTH_POISON, dtype=torch.int32, device=ctx.device)
            geo.DrawSceneToShadowMap(cb, m, *bias)
            assert status(ctx, built_lib) == 0
            maps.append(bits(m))
        assert np.array_equal(maps[0], maps[1]) and np.array_equal(maps[0], ref["depth"]), (bias, int((maps[0] != ref["depth"]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("mix", [gf.MIXED, gf.ALL_F16], ids=["mixed", "f16"])
@pytest.mark.parametrize("name", ["sampler", "texc"])
def test_gbuffer_formats(ctx, built_lib, oracle, name, mix):
    """crychic_draw_gbuffer_formats: a half4 plane holds the oracle's fp32 plane rounded to nearest even (numpy's astype(float16),
    the conversion of float_to_half).  mixed: G0 float4, G1 and G2 half4; f16: all three half4."""
    half = tuple(bool(mix & bit) for bit in (gf.G0_F16, gf.G1_F16, gf.G2_F16))
    case = shade.get(name)
    geo, cb, W, H = geometry(ctx, case), pass_cb(built_lib, case), case["W"], case["H"]
    nd, gb = reference(oracle, case, 1), reference(oracle, case, 2)
    with np.errstate(over="ignore"):
        expect = dict(gb, **{"g%d" % k: gb["g%d" % k].astype(np.float16) for k in range(3) if half[k]})
    for which in ("gbuffer", "fused"):
        check_planes(run_pass(ctx, built_lib, geo, cb, which, W, H, half=half), nd, expect, which)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sampler", "texc"])
def test_two_strips_split_on_an_odd_row(ctx, built_lib, oracle, name):
    """The frame as two strips of G-buffer rows whose boundary is an odd row (the one with the most covered pixels on both sides of
    it): the 2 x 2 quads of the rows on either side of it straddle the strips, and their gradients must still come from the whole quad.  Inside a strip the planes equal the unscissored
    oracle; outside it the poison survives (in depth too for the G-buffer-only entry; the fused entry renders depth and normals
    for the whole frame)."""
    case = shade.get(name)
    geo, cb, W, H = geometry(ctx, case), pass_cb(built_lib, case), case["W"], case["H"]
    nd, gb = reference(oracle, case, 1), reference(oracle, case, 2)
    covered = (gb["depth"] < 0xFFFFFF).sum(axis=1)
    odd = np.arange(1, H - 1, 2)                                       # rows cut - 1 (even) and cut (odd) are one row of quads
    cut = int(odd[np.argmax(np.minimum(covered[odd - 1], covered[odd]))])
    assert cut % 2 == 1 and min(covered[cut - 1], covered[cut]) > W // 4
    for r0, rn in ((0, cut), (cut, H - cut)):
        inside = np.zeros(H, bool); inside[r0:r0 + rn] = True
        for which in ("gbuffer", "fused"):
            out = run_pass(ctx, built_lib, geo, cb, which, W, H, rows=(r0, rn))
            for k in ("g0", "g1", "g2"):
                assert np.array_equal(out[k][inside], bits(gb[k])[inside]), (which, r0, rn, k)
                assert (out[k][~inside] == G_POISON).all(), (which, r0, rn, k)
            if which == "gbuffer":
                assert np.array_equal(out["depth"][inside], gb["depth"][inside]) and (out["depth"][~inside] == DEPTH_POISON).all(), (r0, rn)
            else:
                assert np.array_equal(out["depth"], nd["depth"]) and np.array_equal(out["normal"], bits(nd["normal"])), (r0, rn)
