"""Frames with SIGNALING NaNs in the caller-owned planes (TEST INFRASTRUCTURE ONLY).  fuzz_util.random_case writes np.nan -- quiet --
only, while csrc/devmath.hpp's clamp_len2 and texel_index (v_med3_f32) and saturate (v_max_f32 behind the compiler's quieting) rest on
"the argument is an arithmetic result, never a signaling NaN".  The planes are raw bits the caller owns, so a signaling pattern can sit
in any texel: these frames put some there, inside pixel quads and blur windows, and the host and device tests run SSAO and the lighting
entries over them against the oracle and the features' checkers.  random_case itself is untouched, so every seed keeps its draws."""
import functools

import numpy as np

import fuzz_util
import oracle_lib

SIZES = [(66, 38), (130, 70)]
HALF_PATTERNS = np.array([0x7C01, 0xFE00], np.uint16)
FLOAT_PATTERNS = np.array([0x7F800001, 0xFFA00000, 0x7FBFFFFF], np.uint32)
SHARE = 0.02


def _is_nan32(u):
    return (u & 0x7FFFFFFF) > 0x7F800000


def _is_snan32(u):
    return _is_nan32(u) & ((u & 0x00400000) == 0)


def spoiled_case(size, built_lib):
    """random_case at `size` with about 2 % of the texels of normal, g0, g1 and g2 each given a pattern above in one component (any
    of x, y, z of the normal; any of the four of a G-buffer texel); SSAO on, blurCount 2.  Returns (W, H, planes, constants, knobs)."""
    W, H, planes, c, knobs = fuzz_util.random_case(4200 + size[0], built_lib, size=size)
    planes = {k: np.array(v) for k, v in planes.items()}
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    ys, xs = np.nonzero(rng.random((H, W)) < SHARE)
    planes["normal"].view(np.uint16)[ys, xs, rng.integers(0, 3, len(ys))] = rng.choice(HALF_PATTERNS, len(ys))
    for k in ("g0", "g1", "g2"):
        ys, xs = np.nonzero(rng.random((H, W)) < SHARE)
        planes[k].view(np.uint32)[ys, xs, rng.integers(0, 4, len(ys))] = rng.choice(FLOAT_PATTERNS, len(ys))
    knobs = dict(knobs, ssao_on=True, blurCount=2)
    return W, H, planes, c, knobs


def only_signaling(planes):
    """Covered pixels whose own G-buffer texels hold a signaling NaN and no quiet one."""
    bits = np.concatenate([planes[k].view(np.uint32) for k in ("g0", "g1", "g2")], axis=-1)
    covered = (planes["depth"] & 0xFFFFFF) < 0xFFFFFF
    return covered & _is_snan32(bits).any(-1) & ~(_is_nan32(bits) & ~_is_snan32(bits)).any(-1)


def half_mix(planes):
    """The all-half mix of the frame: numpy's conversion quiets a NaN, so the signaling half patterns are put back where the float
    planes held a signaling NaN.  Returns (packed planes, the float planes a checker is run on: the packed ones widened)."""
    import gbuffer_f16_lib as gf
    packed = gf.pack_planes(planes, gf.ALL_F16)
    rng = np.random.default_rng(16)
    for k in ("g0", "g1", "g2"):
        at = _is_snan32(planes[k].view(np.uint32))
        packed[k] = np.array(packed[k])
        packed[k].view(np.uint16)[at] = rng.choice(HALF_PATTERNS, int(at.sum()))
    assert ((packed["g2"].view(np.uint16) & 0x7FFF) == 0x7C01).any()
    return packed, gf.widen_planes(packed)


@functools.lru_cache(None)
def reference(size, built_lib):
    """The frame and everything the oracle and the checkers say about it, computed once for the host test and its device twin:
    W, H, planes, c, knobs; ao; plain / chain: (RGBA8, radiance) of the plain entry without and with the cube map's mip chain;
    spec: of the gloss + SH + split-sum call (no ambient map, like the features' own tests); half: of the plain entry on the all-half
    mix; and the arguments those calls take."""
    import env_brdf_lib
    import env_sh_lib
    from crychic_renderer_amd import geometry as g
    from test_env_brdf_host import spec_flags
    orc = oracle_lib.load()
    W, H, planes, c, knobs = spoiled_case(size, built_lib)
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    r = dict(W=W, H=H, planes=planes, c=c, knobs=knobs, pcb=pcb)
    r["ao"] = ao = orc.compute_ssao(scb, planes["normal"], planes["depth"], planes["randvec"], 2)
    ndl, radius, sky = knobs["numDirLights"], knobs["pcfSearchRadius"], bool(knobs["sky"])

    def plain(p, cube, **kw):
        return orc.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], ao, p["shadow"], cube, ndl, radius, sky=sky, want_radiance=True, **kw)
    r["plain"] = plain(planes, planes["cube"])
    chain, levels = g.cube_mip_chain(planes["cube"])
    r["chain_cube"], r["chain_kw"] = chain, dict(cube_dim=int(planes["cube"].shape[1]), cube_levels=levels)
    r["chain"] = plain(planes, chain, **r["chain_kw"])
    eb, es = env_brdf_lib.load(), env_sh_lib.load()
    r["spec_planes"] = q = dict(planes, cube=env_brdf_lib.with_table(chain, r["chain_kw"]["cube_dim"], levels, eb.table()[0], es.project(planes["cube"])))
    r["spec_flags"] = knobs["sky"] | spec_flags(levels, True)
    r["spec"] = eb.checker_light(pcb, q, None, ndl, radius, r["spec_flags"], cube_dim=r["chain_kw"]["cube_dim"])
    r["half_planes"], wide = half_mix(planes)
    r["half"] = plain(wide, planes["cube"])
    # the bite: a pixel whose only NaN input is signaling, with a finite radiance by the definition -- had a signaling NaN a way
    # of its own through the kernels, this is where it would show
    only = only_signaling(planes)
    r["bite"] = int((only & np.isfinite(r["plain"][1]).all(-1)).sum())
    return r
