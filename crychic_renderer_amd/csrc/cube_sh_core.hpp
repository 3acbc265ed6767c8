// cube_sh_core.hpp -- the bodies of crychic_project_cube_sh (cube_sh.hip), written so that a host compiler
// builds them too (tests/env_sh_host).
//
// Definition (include/crychic_hip.h "SH9 irradiance"): every texel of the level contributes ten 32-bit integers -- its weight and
// its nine weighted monomials, in units of 2^-20 -- and the level's 28 sums (27 colour sums and the weight sum) are 64-bit integers.
// Integer addition is associative, so a lane, a wavefront, a workgroup and the whole grid may add their texels in any order and
// any grouping: the sums, and with them the coefficient block, are the same bits.  What is rounded is rounded once per texel
// (cube_sh_terms) and once per coefficient (cube_sh_coefficient), both the same on the host.
#pragma once
#include "cube_prefilter_core.hpp"

namespace cry {

constexpr uint32_t kCubeShThreads = 256u;
constexpr uint32_t kCubeShMaxBlocks = 256u;          // the accumulate launch's grid is capped: one wave of workgroups on 256 CUs
constexpr uint32_t kCubeShSums = 28u;                // S_{m,c} at 3 m + c, S_w at 27
constexpr uint32_t kCubeShCoeffBytes = 144u;         // nine float4; the accumulators follow them in the tail


// The nine monomials of a unit vector, in the definition's order.
struct ShBasis { float b[9]; };
CRY_HD ShBasis sh_basis(f3 n)
{
    return ShBasis{ { 1.0f, n.y, n.z, n.x, n.x * n.y, n.y * n.z, fma(3.0f * n.z, n.z, -1.0f), n.x * n.z, fma(n.x, n.x, -(n.y * n.y)) } };
}

// One texel's quantised terms: q[m] = rint((w b_m) 2^20), qw = rint(w 2^20).  r2 is in [1, 3], so w <= 1 and |b_m| <= 2: |q| <= 2^21.
struct CubeShTerms { int32_t q[9]; int32_t qw; };
CRY_HD CubeShTerms cube_sh_terms(uint32_t face, uint32_t x, uint32_t y, uint32_t d)
{
    const f3 dir = cube_texel_direction(face, x, y, d);
    const float r2 = dot3(dir, dir);
    const float len = sqrt_clamped(r2);
    const f3 n = normalize3(dir);
    const float w = rcp(r2 * len);
    const ShBasis B = sh_basis(n);
    CubeShTerms t;
#pragma unroll
    for (int m = 0; m < 9; ++m) t.q[m] = (int32_t)__builtin_rintf((w * B.b[m]) * 1048576.0f);
    t.qw = (int32_t)__builtin_rintf(w * 1048576.0f);
    return t;
}

// Adds texel `idx` of the level (face-major, then rows; idx < 6 d^2) to the 28 sums s.
CRY_HD void cube_sh_accumulate(const uint32_t* __restrict__ level, uint32_t d, uint32_t idx, int64_t (&s)[kCubeShSums])
{
    const uint32_t dd = d * d;
    const uint32_t face = idx / dd, in = idx - face * dd, y = in / d, x = in - y * d;
    const CubeShTerms t = cube_sh_terms(face, x, y, d);
    const uint32_t texel = level[idx];
    const int32_t r = (int32_t)(texel & 255u), g = (int32_t)((texel >> 8) & 255u), b = (int32_t)((texel >> 16) & 255u);
#pragma unroll
    for (int m = 0; m < 9; ++m) {
        s[3 * m] += (int64_t)(t.q[m] * r);            // |q| * 255 < 2^29: the product fits 32 bits
        s[3 * m + 1] += (int64_t)(t.q[m] * g);
        s[3 * m + 2] += (int64_t)(t.q[m] * b);
    }
    s[27] += (int64_t)t.qw;
}

// K_m = 4 pi c_m^2 A_l: all exact in binary
static constexpr double kCubeShK[9] = { 1.0, 2.0, 2.0, 2.0, 3.75, 3.75, 0.3125, 3.75, 0.9375 };
// Coefficient `i` of the block's 36 floats (i = 4 m + c) from the finished sums: C_{m,c}, and 0 for the fourth components.
CRY_HD float cube_sh_coefficient(const int64_t* __restrict__ sums, uint32_t i)
{
    const uint32_t m = i >> 2, c = i & 3u;
    if (c == 3u) return 0.0f;
    return (float)((double)sums[3u * m + c] * kCubeShK[m] / ((double)sums[27] * 255.0));
}

}  // namespace cry
