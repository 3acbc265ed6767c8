"""The G-buffer plane formats' test helpers (TEST INFRASTRUCTURE ONLY): the format bits and the planes of a frame packed into and
widened from a format mix.  The product's format-aware load, light_pixel and resolve run on the host in tests/hostsim
(hostsim_lib: light_frame and rasterize take the formats).  There is no checker library of its own: the contract is stated against
the frozen checkers on the WIDENED planes (oracle_lib, local_light_lib, point_shadow_lib) and against numpy.float16 of the oracle
rasteriser's fp32 planes."""
import numpy as np

G0_F16, G1_F16, G2_F16 = 0x1000, 0x2000, 0x4000          # CRYCHIC_GBUFFER_G*_F16
F16_MASK = 0x7000
MIXES = [m << 12 for m in range(8)]                      # all eight format mixes, as flag bits
MIXED, ALL_F16 = G1_F16 | G2_F16, F16_MASK               # "mixed": G0 float4, G1 + G2 half4; "f16": all three half4


def pack_planes(p, mix):
    """The planes of p with G0..G2 stored in the formats of `mix`: a half plane is numpy's float32 -> float16 conversion (round to
    nearest even, subnormals kept, overflow to infinity -- tests/test_gbuffer_f16_host.py holds it against float_to_half)."""
    q = dict(p)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(3):
            g = np.ascontiguousarray(p["g%d" % k], np.float32)
            q["g%d" % k] = g.astype(np.float16) if mix & (G0_F16 << k) else g
    return q


def widen_planes(p):
    """The planes of p with every G-buffer plane as float32 (a half plane widens exactly): what the frozen checkers are run on."""
    q = dict(p)
    for k in range(3):
        q["g%d" % k] = np.ascontiguousarray(p["g%d" % k]).astype(np.float32)
    return q


def mix_of(p):
    """The CRYCHIC_GBUFFER_* bits of the planes' dtypes."""
    return sum((G0_F16 << k) for k in range(3) if p["g%d" % k].dtype == np.float16)
