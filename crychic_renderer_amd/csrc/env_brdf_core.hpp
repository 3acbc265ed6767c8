// env_brdf_core.hpp -- the bodies of crychic_build_env_brdf (env_brdf.hip), written so that a host compiler
// builds them too (tests/env_brdf_host).
//
// Definition (include/crychic_hip.h "environment BRDF table"): texel (row j, column i) of the 32 x 32 table is the second factor of
// the split sum at roughness (j + 0.5) / 32 and N.V = (i + 0.5) / 32: the integral of the pass's own specular BRDF -- NDF_GGX with
// a^2 = rho^2 as the sampled lobe, GeometrySmith with k = (rho + 1)^2 / 8 -- over that lobe, split into the factor of R0 (A) and the
// Fresnel offset (B).  The quadrature is a fixed product grid of 256 xi x 16 phi; every sample contributes two 32-bit integers in
// units of 2^-24 and the two sums are 64-bit integers.  Integer addition is associative, so a lane, a wavefront or a host loop may
// add the samples in any order and any grouping: the sums, and with them the texel, are the same bits.  What is rounded is rounded
// once per sample (env_brdf_accumulate) and once per texel (env_brdf_pack), both the same on the host.
#pragma once
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kEnvBrdfDim = 32u;                // rows (roughness) and columns (N.V)
constexpr uint32_t kEnvBrdfXi = 256u;                // xi_s = (s + 0.5) / 256
constexpr uint32_t kEnvBrdfPhi = 16u;                // phi_t = pi (t + 0.5) / 16: the half circle, V in the xz-plane

// cos(phi_t), the definition's constants: RN(cos(pi (t + 0.5) / 16)) for t = 0 .. 7, their negations in reverse for t = 8 .. 15
#define CRY_ENV_BRDF_F(bits) __builtin_bit_cast(float, (uint32_t)(bits))
static constexpr float kEnvBrdfCos[kEnvBrdfPhi] = {
    CRY_ENV_BRDF_F(0x3f7ec46du), CRY_ENV_BRDF_F(0x3f74fa0bu), CRY_ENV_BRDF_F(0x3f61c598u), CRY_ENV_BRDF_F(0x3f45e403u),
    CRY_ENV_BRDF_F(0x3f226799u), CRY_ENV_BRDF_F(0x3ef15aeau), CRY_ENV_BRDF_F(0x3e94a031u), CRY_ENV_BRDF_F(0x3dc8bd36u),
    CRY_ENV_BRDF_F(0xbdc8bd36u), CRY_ENV_BRDF_F(0xbe94a031u), CRY_ENV_BRDF_F(0xbef15aeau), CRY_ENV_BRDF_F(0xbf226799u),
    CRY_ENV_BRDF_F(0xbf45e403u), CRY_ENV_BRDF_F(0xbf61c598u), CRY_ENV_BRDF_F(0xbf74fa0bu), CRY_ENV_BRDF_F(0xbf7ec46du) };
#undef CRY_ENV_BRDF_F

// What every sample of texel (j, i) shares.
struct EnvBrdfTexel { float a2m1, k, omk, vz, vx, gV; };
CRY_HD EnvBrdfTexel env_brdf_texel(uint32_t j, uint32_t i)
{
    const float rho = ((float)j + 0.5f) * 0.03125f, mu = ((float)i + 0.5f) * 0.03125f;      // both exact
    EnvBrdfTexel T;
    T.a2m1 = fma(rho, rho, -1.0f);
    T.k = 0.125f * (rho + 1.0f) * (rho + 1.0f);         // PBR.hlsl:34, that product order
    T.omk = 1.0f - T.k;
    T.vz = mu;
    T.vx = len_from_sq(fma(-mu, mu, 1.0f));
    T.gV = rcp(fma(T.vz, T.omk, T.k));
    return T;
}

// Adds the sixteen samples (s, t = 0 .. 15) of the texel to its two sums.  Every term is below 19.5, so q < 2^29 fits 32 bits; a
// sample whose light direction is not above the surface contributes nothing (selected before the conversion: no NaN reaches it).
CRY_HD void env_brdf_accumulate(const EnvBrdfTexel& T, uint32_t s, int64_t& SA, int64_t& SB)
{
    const float xi = ((float)s + 0.5f) * 0.00390625f;   // exact
    const float c2 = (1.0f - xi) * rcp(fma(T.a2m1, xi, 1.0f));
    const float c = len_from_sq(c2);
    const float sn = len_from_sq(1.0f - c2);
    const float rc = rcp(c);
#pragma unroll
    for (uint32_t t = 0; t < kEnvBrdfPhi; ++t) {
        const float voh = fma(T.vx, sn * kEnvBrdfCos[t], T.vz * c);
        const float lz = fma(2.0f * voh, c, -T.vz);
        const bool above = lz > 0.0f;
        const float gL = lz * rcp(fma(lz, T.omk, T.k));
        const float gv = ((T.gV * gL) * voh) * rc;
        const float f = 1.0f - saturate(voh);
        const float fc = f * f * f * f * f;
        const float tB = fc * gv;
        const float tA = (1.0f - fc) * gv;
        SA += (int64_t)(int32_t)__builtin_rintf((above ? tA : 0.0f) * 16777216.0f);
        SB += (int64_t)(int32_t)__builtin_rintf((above ? tB : 0.0f) * 16777216.0f);
    }
}

// The texel of finished sums: A | B << 16, two R16 UNORM values of the means over the 4096 samples (2^24 * 4096 = 2^36).  |S| < 2^42:
// the conversion to double and the scaling are exact, the conversion to binary32 is correctly rounded.
CRY_HD uint32_t env_brdf_pack(int64_t SA, int64_t SB)
{
    const float A = (float)((double)SA * 1.4551915228366852e-11), B = (float)((double)SB * 1.4551915228366852e-11);     // 2^-36
    return float_to_unorm16(A) | (float_to_unorm16(B) << 16);
}

}  // namespace cry
