"""The tiled cull of the local lights on the device: the frames and light sets of tests/test_light_cull_host.py (thinned non-finite
world positions, 1024 point + 1024 spot lights; tests/light_cull_cases.py) through crychic_deferred_light_spots,
crychic_deferred_light_spots_shadowed, crychic_deferred_light_point_shadows and the flagged calls that land in
light_general_local_kernel, whole frame and row ranges, against the frozen checkers: RGBA8 bit-equal, radiance equal up to NaN
payloads.  One coherent or incoherent frame per family (the CPU tier runs both), and the light counts 33, 257 and 1024."""
import numpy as np
import pytest

import fuzz_util
import gbuffer_f16_lib as gf
import light_cull_cases as lc
from local_lights_util import _dev_lights
from test_point_shadows import _light, _point_desc, _spot_desc

pytestmark = pytest.mark.gpu

# the entry a family's call goes through; the flagged families (half G0, gloss, SH) land in light_general_local_kernel whatever the entry
ENTRY = {"points": "spots", "points_spots": "spots", "spot_shadows": "spots_shadowed", "point_shadows": "point_shadows",
         "point_spot_shadows": "point_shadows", "g0_half": "point_shadows", "gloss": "point_shadows", "gloss_sh": "spots_shadowed",
         "cube_chain": "spots"}


def _to_dev(ctx, a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.view(np.int16) if a.dtype == np.uint16 else a).to(ctx.device)


def _run_on_device(built_lib, case, entry, ranges):
    """The case through `entry`: the whole frame, then `ranges` into a second pair of targets.  Returns [(RGBA8, radiance)] * 2."""
    import torch
    from crychic_renderer_amd import Context
    ctx = Context(0)
    try:
        dev = {k: _to_dev(ctx, v) for k, v in case.planes.items()}
        dp, ds = _dev_lights(ctx, case.kw.get("points")), _dev_lights(ctx, case.kw.get("spots"))
        maps = _to_dev(ctx, case.kw["maps"]) if "maps" in case.kw else None
        cubes = _to_dev(ctx, case.kw["cubes"]) if "cubes" in case.kw else None
        sdesc = _spot_desc(maps) if maps is not None else None
        pdesc = _point_desc(cubes, case.kw["projs"]) if cubes is not None else None
        ao = _to_dev(ctx, case.ambient) if case.ambient is not None else None
        args = dict(ndl=case.ndl, radius=case.radius, ambient=ao, entry=entry, shadow_dim=int(case.planes["shadow"].shape[1]),
                    cube_dim=int(case.kw.get("cube_dim", 0)) or int(case.planes["cube"].shape[1]))
        flags = case.flags | gf.mix_of(case.planes)
        W, H = case.W, case.H
        rc, out, rad = _light(built_lib.lib, ctx, case.cb, dev, W, H, flags, dp, ds, sdesc, pdesc, **args)
        built_lib.check(rc)
        out2, rad2 = torch.zeros_like(out), torch.zeros_like(rad)
        for r0, rn in ranges:
            built_lib.check(_light(built_lib.lib, ctx, case.cb, dev, W, H, flags, dp, ds, sdesc, pdesc, row0=r0, rows=rn, out=out2, rad=rad2, **args)[0])
        torch.cuda.synchronize()
        return [(o.cpu().numpy(), r.cpu().numpy()) for o, r in ((out, rad), (out2, rad2))]
    finally:
        ctx.close()


def _same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), (what, int((got[0] != ref[0]).any(-1).sum()))
    assert fuzz_util.same_floats(got[1], ref[1]), what


@pytest.mark.parametrize("family", list(lc.FAMILIES))
def test_fuzz_frame_on_device_equals_checker(built_lib, family):
    """One frame of the family's case set: the whole frame and the three row ranges (the last anchored off the tile grid) == the
    checker."""
    k = list(lc.FAMILIES).index(family)
    seed = lc.seeds_of(family)[(k // 2) % 2]            # coherent and incoherent frames, with and without infinite FalloffEnd, in turn
    case = lc.Case(family, seed, built_lib)
    whole, strips = _run_on_device(built_lib, case, ENTRY[family], fuzz_util.CULL_ROW_RANGES)
    ref = case.reference()
    _same(whole, ref, (family, seed, "whole frame"))
    _same(strips, ref, (family, seed, "row ranges"))


@pytest.mark.parametrize("n", [33, 257, 1024])
def test_light_counts_on_device(built_lib, n):
    """n point and n spot lights of which the last alone reaches one tile (test_light_cull_host.count_case): mask words 1, 8 and 31,
    the second trip of the cull loop, the last bit of the last word."""
    from test_light_cull_host import count_case
    case, _ = count_case("points_spots", n, built_lib)
    whole, _ = _run_on_device(built_lib, case, "spots", ())
    _same(whole, case.reference(), n)
