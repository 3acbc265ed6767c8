// cube_prefilter_core.hpp -- the per-texel body of crychic_prefilter_cube_chain (cube_prefilter.hip), written so
// that a host compiler builds it too (tests/gloss_host).
//
// Definition (include/crychic_hip.h "prefiltered chain"): texel (x, y) of face f of level k >= 1 of the destination is the weighted
// mean of the SOURCE chain, looked up with the lighting pass's own trilinear sampler (cube_trilinear<true>) along the kept
// directions of the level's sample table, in index order:  acc = fma(lz_i, c_i, acc);  texel = float_to_unorm8(acc * rcpW).
// The table (host_constants.cpp, crychic_cube_prefilter_samples) is the same for every texel of a level, so its entries -- and with
// them the two source levels, their sizes and offsets and the mix factor of a sample -- are wave-uniform: scalar loads and scalar
// arithmetic.  What is per lane is the frame (N, T, B), the direction, the two face footprints and the filter.
#pragma once
#include "light_core.hpp"

namespace cry {

constexpr uint32_t kCubePrefilterSamples = 32u;
constexpr uint32_t kCubePrefilterThreads = 256u;

// A level's table as the kernel takes it, by value in the kernarg segment (528 bytes): entry i = { lx, ly, lz, lod }.
struct CubePrefilterTable {
    float s[kCubePrefilterSamples][4];
    uint32_t count;
    float rcpW;
};

// The direction of the centre of texel (x, y) of face f of a d x d level: the inverse of cube_level_address's face table, with
// face coordinates (s, t) = ((2x + 1) / d - 1, (2y + 1) / d - 1) and major axis 1.
CRY_HD f3 cube_texel_direction(uint32_t face, uint32_t x, uint32_t y, uint32_t d)
{
    const float rd = rcp((float)d);
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
// a x b, each component one fma(a, b, -(c d))
CRY_HD f3 cross3(f3 a, f3 b)
{
    return f3{ fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x)) };
}

// One texel of level k (d x d, d = cube_level_dim(dim, k)) of the prefiltered chain.  src: the whole source chain (dim, levels).
// Texels are finite and the directions never degenerate (|N| = 1, |l| = 1, lz > 0), so there is no NaN case.
CRY_HD uint32_t cube_prefilter_texel(const uint32_t* __restrict__ src, uint32_t dim, uint32_t levels, uint32_t d, uint32_t face,
                                     uint32_t x, uint32_t y, const CubePrefilterTable& tab)
{
    const f3 N = normalize3(cube_texel_direction(face, x, y, d));
    const f3 up = __builtin_fabsf(N.z) < 0.999f ? f3{ 0.0f, 0.0f, 1.0f } : f3{ 1.0f, 0.0f, 0.0f };
    const f3 T = normalize3(cross3(up, N));
    const f3 B = cross3(N, T);
    auto fetch = [&](uint32_t i) {
        const float lx = tab.s[i][0], ly = tab.s[i][1], lz = tab.s[i][2];
        const f3 L{ fma(lz, N.x, fma(ly, B.x, lx * T.x)), fma(lz, N.y, fma(ly, B.y, lx * T.y)), fma(lz, N.z, fma(ly, B.z, lx * T.z)) };
        return cube_trilinear_fetch(src, dim, levels, L, tab.s[i][3]);
    };
    f4 acc{ 0.0f, 0.0f, 0.0f, 0.0f };
    CubeTrilinearFetch cur = fetch(0u);
    for (uint32_t i = 0; i < tab.count; ++i) {
        // the last iteration fetches its own sample again: in range, and nothing reads it
        const CubeTrilinearFetch nxt = fetch(i + 1u < tab.count ? i + 1u : i);
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_sched_barrier(0);          // the next sample's four loads are issued before this sample's filter waits
#endif
        const f4 c = cube_trilinear_resolve<true>(cur);
        const float w = tab.s[i][2];
        acc = f4{ fma(w, c.x, acc.x), fma(w, c.y, acc.y), fma(w, c.z, acc.z), fma(w, c.w, acc.w) };
        cur = nxt;
    }
    return float_to_unorm8(acc.x * tab.rcpW) | (float_to_unorm8(acc.y * tab.rcpW) << 8) | (float_to_unorm8(acc.z * tab.rcpW) << 16) |
           (float_to_unorm8(acc.w * tab.rcpW) << 24);
}

// Thread `idx` of the launch of level k: texel idx of the level (face-major, then rows), or nothing past the level's 6 d^2 texels.
CRY_HD void cube_prefilter_thread(const uint32_t* __restrict__ src, uint32_t* __restrict__ dstLevel, uint32_t dim, uint32_t levels, uint32_t d,
                                  uint32_t idx, const CubePrefilterTable& tab)
{
    const uint32_t dd = d * d;
    if (idx >= 6u * dd) return;
    const uint32_t face = idx / dd, in = idx - face * dd, y = in / d, x = in - y * d;
    dstLevel[idx] = cube_prefilter_texel(src, dim, levels, d, face, x, y, tab);
}

}  // namespace cry
