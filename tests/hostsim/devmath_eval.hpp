// devmath_eval.hpp -- TEST HARNESS ONLY.  One primitive of csrc/devmath.hpp per `kind` (the numbering of or_eval_array,
// oracle/or_light.c), for the host build (tests/hostsim hs_eval_array) and the device build (tests/devmath_dev dm_eval_array) alike:
// the two tiers differ in what the compiler makes of devmath.hpp, never in which primitive a kind names.
// Arguments and results travel as bit patterns: an integer argument is the bits of `a` / `b`, an integer result is returned as is.
#pragma once
#include "devmath.hpp"

namespace cry {

// (w, h) of the bilinear set-up kinds 35 + 4 s + o
CRY_HD uint32_t devmath_eval_size(int s, int which)
{
    const uint32_t w = s == 0 ? 2u : s == 1 ? 16u : s == 2 ? 130u : 16384u;
    const uint32_t h = s == 0 ? 16u : s == 1 ? 130u : s == 2 ? 16384u : 2u;
    return which ? h : w;
}

CRY_HD uint32_t devmath_eval(int kind, float a, float b)
{
    const uint32_t ua = f2u(a), ub = f2u(b);
    switch (kind) {
    case 0: return f2u(det_sin(a));
    case 1: return f2u(det_cos(a));
    case 2: return f2u(det_log2(a));
    case 3: return f2u(det_exp2(a));
    case 4: return f2u(det_pow(a, b));
    case 6: return f2u(d24_to_float(ua));
    case 7: return f2u(unorm16_to_float(ua & 0xFFFFu));
    case 8: return f2u(unorm8_to_float(ua & 0xFFu));
    case 9: return f2u(half_to_float((uint16_t)ua));
    case 10: return f2u(pow_inv_gamma(a));
    case 11: return f2u(pow_inv_gamma2(v2f{ b, a }).y);
    case 12: return f2u(rcp(a));
    case 13: return f2u(rcp_normal(a));
    case 14: return f2u(divf(a, b));
    case 15: return f2u(clamp_len2(a));
    case 16: return f2u(sqrt_clamped(a));
    case 17: return f2u(len_from_sq(a));
    case 18: return f2u(inv_len_from_sq(a));
    case 19: return f2u(rcp2(v2f{ a, b }).x);
    case 20: return f2u(rcp2(v2f{ b, a }).y);
    case 21: return f2u(rcp_normal2(v2f{ a, b }).x);
    case 22: return f2u(rcp_normal2(v2f{ b, a }).y);
    case 23: return f2u(inv_len_from_sq2(v2f{ a, b }).x);
    case 24: return f2u(inv_len_from_sq2(v2f{ b, a }).y);
    case 25: return f2u(pow_inv_gamma2(v2f{ a, b }).x);
    case 26: return f2u(saturate(a));
    case 27: return f2u(maxnn(a, b));
    case 28: return f2u(sign1(a));
    case 29: return f2u(signf(a));
    case 30: return f2u(lerpf(a, b, 0.37f));
    case 31: return f2u(lerpf(0.04f, b, a));
    case 32: return float_to_unorm8(a);
    case 33: return float_to_unorm16(a);
    case 34: return (uint32_t)texel_index(a, ub);
    case 51: return mul24(ua, ub);
    default: break;
    }
    if (kind >= 35 && kind < 51) {
        const int s = (kind - 35) >> 2;
        const Bilin q = bilinear_setup<false>(a, b, devmath_eval_size(s, 0), devmath_eval_size(s, 1));
        switch ((kind - 35) & 3) {
        case 0: return (uint32_t)q.i0;
        case 1: return (uint32_t)q.j0;
        case 2: return f2u(q.fx);
        default: return f2u(q.fy);
        }
    }
    return 0u;
}

CRY_HD bool devmath_eval_has(int kind) { return kind >= 0 && kind < 52 && kind != 5; }

}  // namespace cry
