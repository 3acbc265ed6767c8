// sky_core.hpp -- the body of crychic_render_sky and of crychic_sky_sun_colour (include/crychic_hip.h states the definition; DESIGN.md
// section 29), built for the device (sky.hip) and for the host (api.cpp for the sun's colour; tests/sky_host).  One lane per texel of
// level 0 of a cube map, an 8 x 8 texel tile per wavefront: the texel centre's ray is marched through a single-scattering atmosphere
// in viewSteps samples, each with a march of sunSteps samples towards the sun, and the radiance is tone-mapped into RGBA8.
//
// What the lanes of a tile share is shared through votes, never through data:
//   * a view sample whose sun ray the planet blocks in every lane skips its sun march (night, and the lower part of twilight);
//   * the ground term runs only in a wave with a lane whose ray ends on the ground, the sun's disc only in one with a lane inside it.
// A vote only skips work whose result would not be used (every use is selected by the lane's own predicate), so the host build, whose
// vote is the lane's own predicate, computes the same bits.  Both loops run viewSteps and sunSteps times in every lane.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kSkyMaxViewSteps = 64u, kSkyMaxSunSteps = 32u;      // CRYCHIC_SKY_MAX_VIEW_STEPS, CRYCHIC_SKY_MAX_SUN_STEPS
// a wavefront covers an 8 x 8 texel tile (lane = 8 y + x), a workgroup four tiles side by side: 32 x 8 texels
constexpr uint32_t kSkyTile = 8u, kSkyWaves = 4u, kSkyGroupW = kSkyTile * kSkyWaves, kSkyThreads = 64u * kSkyWaves;
CRY_HD uint32_t sky_lane_x(uint32_t thread) { return (thread >> 6) * kSkyTile + (thread & (kSkyTile - 1u)); }     // within the workgroup
CRY_HD uint32_t sky_lane_y(uint32_t thread) { return (thread >> 3) & (kSkyTile - 1u); }

// the atmosphere (kilometres), the header's constants
constexpr float kSkyRg = 6360.0f, kSkyRg2 = 40449600.0f, kSkyInvRg = 0.000157232702f;
constexpr float kSkyNegInvHR = -0.180336878f, kSkyNegInvHM = -1.20224583f;             // -log2(e) / 8, -log2(e) / 1.2
constexpr float kSkyBetaR[3] = { 5.8e-3f, 13.5e-3f, 33.1e-3f }, kSkyBetaM = 21.0e-3f;
constexpr float kSkyTauR[3] = { 0.00836763065f, 0.0194763839f, 0.0477532074f }, kSkyTauM = 0.0333262533f;   // beta log2(e); Mie: 1.1 beta
constexpr float kSkyPhaseR = 0.0596831031f, kSkyPhaseM = 0.0195609424f;                // 3 / (16 pi), 3 (1 - g^2) / (8 pi (2 + g^2))
constexpr float kSkyG2 = -1.52f, kSkyOnePlusG2 = 1.5776f;                              // -2 g, 1 + g^2
constexpr float kSkyInvPi = 0.318309873f;

struct SkyParams {      // crychic_sky_params
    float sunDir[3], altitude, sunIntensity, exposure, sunAngularRadius, groundAlbedo;
    uint32_t viewSteps, sunSteps, reserved[2];
};

// what depends on the parameters alone: computed once on the host, wave-uniform on the device
struct SkyConsts {
    float S[3];             // the unit vector towards the sun
    float a0, cT, r0Sy;     // r0^2 - Rg^2, Rt^2 - r0^2, r0 S.y  (r0 = Rg + altitude: the observer is at (0, r0, 0))
    float r0;
    float invNv, invNv2, invNs, invNs2;
    float cosDisc, sunI, exposure, groundK;
    uint32_t Nv, Ns;
};

inline SkyConsts sky_consts(const SkyParams& p)
{
    SkyConsts k;
    const double x = p.sunDir[0], y = p.sunDir[1], z = p.sunDir[2];
    const double len = __builtin_sqrt(x * x + y * y + z * z);
    k.S[0] = (float)(x / len); k.S[1] = (float)(y / len); k.S[2] = (float)(z / len);
    const double alt = p.altitude;
    const float r0 = 6360.0f + p.altitude;
    k.a0 = (float)(alt * (12720.0 + alt));
    k.cT = (float)((60.0 - alt) * (12780.0 + alt));
    k.r0Sy = r0 * k.S[1];
    k.r0 = r0;
    k.Nv = p.viewSteps; k.Ns = p.sunSteps;
    k.invNv = 1.0f / (float)k.Nv; k.invNv2 = k.invNv * k.invNv;
    k.invNs = 1.0f / (float)k.Ns; k.invNs2 = k.invNs * k.invNs;
    const double a2 = (double)p.sunAngularRadius * (double)p.sunAngularRadius;
    k.cosDisc = (float)(1.0 - a2 * (0.5 - a2 / 24.0));
    k.sunI = p.sunIntensity;
    k.exposure = p.exposure;
    k.groundK = (p.groundAlbedo * kSkyInvPi) * p.sunIntensity;
    return k;
}

// the kernel's arguments (kernarg segment: every field is wave-uniform)
struct SkyArgs {
    uint32_t* cube;
    uint32_t dim, face0, tilesX, groupsPerFace;
    float rd;               // rcp((float)dim)
    SkyConsts k;
};

struct SkyLaunch { SkyArgs args; uint32_t groups; };       // groups == 0: nothing to launch

// The launcher's plan.  The caller has checked every argument (api.cpp).
inline SkyLaunch sky_launch(uint8_t* cube, uint32_t dim, uint32_t face0, uint32_t faces, const SkyParams& p)
{
    SkyLaunch L;
    SkyArgs& a = L.args;
    a.cube = reinterpret_cast<uint32_t*>(cube);
    a.dim = dim; a.face0 = face0;
    a.tilesX = (dim + kSkyGroupW - 1u) / kSkyGroupW;
    a.groupsPerFace = a.tilesX * ((dim + kSkyTile - 1u) / kSkyTile);      // at most 256 * 1024
    a.rd = rcp((float)dim);
    a.k = sky_consts(p);
    L.groups = a.groupsPerFace * faces;
    return L;
}

// det_exp2 of an argument that is never NaN (every quantity of the definition is finite): without its NaN branch, which would split
// the wavefront twice per sun sample
CRY_HD float sky_exp2(float z) { return det_exp2_clamped(clampf(z, -125.0f, 127.0f)); }

// height above the ground of a point with q = r^2 - Rg^2: q * rcp(len_from_sq(q + Rg2) + Rg).  Wherever the result is used the point
// lies between the ground and the shell, q + Rg2 in [4.0e7, 4.2e7]: inside sqrt_clamped's and rcp_normal's domains, so the clamp and the
// select of the general forms are left out (an unlit lane of a mixed wavefront may march through the planet; its sums are discarded)
CRY_HD float sky_height(float q) { return q * rcp_normal(sqrt_clamped(q + kSkyRg2) + kSkyRg); }

// whether the planet stands between a point (q = r^2 - Rg^2, bs = P.S) and the sun
CRY_HD bool sky_blocked(float q, float bs) { return bs < 0.0f && fma(bs, bs, -q) >= 0.0f; }

// the length of a ray's way to the shell from a point with c = Rt^2 - r^2 >= 0 and b = P.dir
CRY_HD float sky_to_shell(float c, float b)
{
    const float sq = len_from_sq(fma(b, b, c));
    return (b >= 0.0f) ? c * rcp(sq + b) : sq - b;
}

struct SkyDepth { float dR, dM; };

// The sun march: the integrals of the two densities from a point (q, bs as above, c = Rt^2 - r^2 >= 0) to the shell, towards the sun.
CRY_HD SkyDepth sky_sun_depth(const SkyConsts& k, float q, float bs, float c)
{
    const float L = sky_to_shell(c, bs);
    const float twob = bs + bs;
    SkyDepth D{ 0.0f, 0.0f };
    for (uint32_t j = 0; j < k.Ns; ++j) {
        const float u = ((float)j + 0.5f) * k.invNs;
        const float s = L * (u * u);
        const float ds = L * ((float)(2u * j + 1u) * k.invNs2);
        const float h = sky_height(fma(s, s + twob, q));
        D.dR = fma(sky_exp2(h * kSkyNegInvHR), ds, D.dR);
        D.dM = fma(sky_exp2(h * kSkyNegInvHM), ds, D.dM);
    }
    return D;
}

// 2^-(tauR_c dR + tauM dM): the transmittance of channel c over the two depths
CRY_HD float sky_transmittance(int c, float dR, float dM) { return sky_exp2(-fma(kSkyTauR[c], dR, kSkyTauM * dM)); }

// crychic_sky_sun_colour
inline void sky_sun_colour(const SkyParams& p, float rgb[3])
{
    const SkyConsts k = sky_consts(p);
    if (sky_blocked(k.a0, k.r0Sy)) { rgb[0] = rgb[1] = rgb[2] = 0.0f; return; }
    const SkyDepth D = sky_sun_depth(k, k.a0, k.r0Sy, k.cT);
    for (int c = 0; c < 3; ++c) rgb[c] = k.sunI * sky_transmittance(c, D.dR, D.dM);
}

CRY_HD f3 sky_texel_direction(uint32_t face, uint32_t x, uint32_t y, float rd)
{
    const float s = (float)(2u * x + 1u) * rd - 1.0f, t = (float)(2u * y + 1u) * rd - 1.0f;
    switch (face) {
    case 0u: return f3{ 1.0f, -t, -s };
    case 1u: return f3{ -1.0f, -t, s };
    case 2u: return f3{ s, 1.0f, t };
    case 3u: return f3{ s, -1.0f, -t };
    case 4u: return f3{ s, -t, 1.0f };
    default: return f3{ -s, -t, -1.0f };
    }
}

// One texel of the cube map.  `any`: a vote over the lanes that run together (the device: the wavefront's active lanes; the host: the
// lane's own predicate).
template <class Any>
CRY_HD uint32_t sky_texel(const SkyConsts& k, uint32_t face, uint32_t x, uint32_t y, float rd, Any any)
{
    const f3 v = normalize3(sky_texel_direction(face, x, y, rd));
    const f3 S{ k.S[0], k.S[1], k.S[2] };
    const float mu = dot3(v, S);
    // the view ray's segment: to the ground if it meets it, else to the shell
    const float b = k.r0 * v.y, twob = b + b;
    const float dg = fma(b, b, -k.a0);
    const bool ground = b < 0.0f && dg >= 0.0f;
    const float tEnd = ground ? k.a0 * rcp(len_from_sq(dg) - b) : sky_to_shell(k.cT, b);
    // the view march
    float vR = 0.0f, vM = 0.0f, sR[3] = { 0.0f, 0.0f, 0.0f }, sM[3] = { 0.0f, 0.0f, 0.0f };
    for (uint32_t i = 0; i < k.Nv; ++i) {
        const float u = ((float)i + 0.5f) * k.invNv;
        const float t = tEnd * (u * u);
        const float dt = tEnd * ((float)(2u * i + 1u) * k.invNv2);
        const float w = t * (t + twob);                 // r^2 - r0^2
        const float q = k.a0 + w;
        const float h = sky_height(q);
        const float rhoR = sky_exp2(h * kSkyNegInvHR) * dt, rhoM = sky_exp2(h * kSkyNegInvHM) * dt;
        const float mR = fma(0.5f, rhoR, vR), mM = fma(0.5f, rhoM, vM);       // the depths up to the sample itself
        vR += rhoR;
        vM += rhoM;
        const float bs = fma(t, mu, k.r0Sy);
        const bool lit = !sky_blocked(q, bs);
        if (any(lit)) {
            const SkyDepth D = sky_sun_depth(k, q, bs, maxnn(k.cT - w, 0.0f));
            const float dR = mR + D.dR, dM = mM + D.dM;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float T = sky_transmittance(c, dR, dM);
                sR[c] = lit ? fma(T, rhoR, sR[c]) : sR[c];
                sM[c] = lit ? fma(T, rhoM, sM[c]) : sM[c];
            }
        }
    }
    // phases and radiance
    const float m1 = fma(mu, mu, 1.0f);
    const float phR = kSkyPhaseR * m1;
    const float xg = fma(kSkyG2, mu, kSkyOnePlusG2);
    const float phM = (kSkyPhaseM * m1) * rcp(xg * len_from_sq(xg));
    float L[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = k.sunI * fma(phR * kSkyBetaR[c], sR[c], (phM * kSkyBetaM) * sM[c]);
    // the ground and the sun's disc, both seen through the whole view ray
    const bool disc = !ground && mu >= k.cosDisc;
    if (any(ground || disc)) {
        const float w = tEnd * (tEnd + twob);
        const float q = maxnn(k.a0 + w, 0.0f);
        const float bs = fma(tEnd, mu, k.r0Sy);
        const bool sunlit = ground && bs > 0.0f;
        SkyDepth D{ 0.0f, 0.0f };
        if (any(sunlit)) D = sky_sun_depth(k, q, bs, maxnn(k.cT - w, 0.0f));
        const float cosG = bs * kSkyInvRg;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float Tv = sky_transmittance(c, vR, vM);
            const float g = ((k.groundK * cosG) * sky_transmittance(c, D.dR, D.dM)) * Tv;
            L[c] = sunlit ? L[c] + g : L[c];
            L[c] = disc ? fma(k.sunI, Tv, L[c]) : L[c];
        }
    }
    // the lighting pass's tone map: pow(x / (x + 1), 1 / 2.2)
    uint32_t o = 0xFF000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float e = L[c] * k.exposure;
        o |= float_to_unorm8(pow_inv_gamma(divf(e, e + 1.0f))) << (8 * c);
    }
    return o;
}

}  // namespace cry
