// env_brdf_host.cpp -- csrc/env_brdf_core.hpp and the SpecularSplitSum instantiations of light_pixel built for the host (TEST
// INFRASTRUCTURE): the bodies of the kernels of env_brdf.hip and of the split-sum variants of light_general.hip, bound through
// light_bind.hpp as the library binds them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "env_brdf_core.hpp"
#include "../hostsim/host_light.hpp"

// The body's two sums of texel (row j, column i) over the sample rows listed in `rows` (each one xi with its sixteen phi), in the
// order given, through env_brdf_accumulate.
extern "C" void bh_sums(uint32_t j, uint32_t i, const uint32_t* rows, uint32_t count, int64_t* sums)
{
    using namespace cry;
    const EnvBrdfTexel T = env_brdf_texel(j, i);
    int64_t a = 0, b = 0;
    for (uint32_t n = 0; n < count; ++n) env_brdf_accumulate(T, rows[n], a, b);
    sums[0] = a; sums[1] = b;
}

// The launch as the device runs it: 1024 wavefronts, lane l of a wavefront takes xi rows 4 l .. 4 l + 3, the lanes' sums are added
// and lane 0 stores the texel.  table: 4096 bytes of whatever; sums (may be null): the 2048 finished sums.
extern "C" void bh_build(uint32_t* table, int64_t* sums)
{
    using namespace cry;
    for (uint32_t texel = 0; texel < kEnvBrdfDim * kEnvBrdfDim; ++texel) {
        const EnvBrdfTexel T = env_brdf_texel(texel / kEnvBrdfDim, texel % kEnvBrdfDim);
        int64_t a = 0, b = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            int64_t la = 0, lb = 0;
            for (uint32_t m = 0; m < kEnvBrdfXi / 64u; ++m) env_brdf_accumulate(T, lane * (kEnvBrdfXi / 64u) + m, la, lb);
            a += la; b += lb;
        }
        table[texel] = env_brdf_pack(a, b);
        if (sums) { sums[2u * texel] = a; sums[2u * texel + 1u] = b; }
    }
}

extern "C" uint32_t bh_pack(const int64_t* sums) { return cry::env_brdf_pack(sums[0], sums[1]); }
extern "C" uint64_t bh_table_offset(uint32_t dim, uint32_t levels) { return cry::env_brdf_offset(dim, levels); }

// The binding's validation of a call with the flag: 0 ok, 1 no gloss chain, 2 null cube map, 3 misaligned table.
extern "C" int bh_check(uint32_t flags, uintptr_t cube, uint32_t cubeDim)
{
    return (int)cry::env_brdf_check(flags, reinterpret_cast<const void*>(cube), cubeDim);
}

// The message the entries report that refusal with, formatted as they format it.
extern "C" int bh_check_message(uint32_t flags, uintptr_t cube, uint32_t cubeDim, char* out, size_t cap)
{
    const cry::EnvBrdfCheck c = cry::env_brdf_check(flags, reinterpret_cast<const void*>(cube), cubeDim);
    return std::snprintf(out, cap, cry::env_brdf_check_message(c), cry::env_brdf_offset(cubeDim, (flags >> 16) & 15u));
}

// Every crychic_deferred_light* entry with CRYCHIC_LIGHT_ENV_BRDF on the host (tests/hostsim/host_light.hpp): the flag maps onto the
// general family, with CubeGloss, SpecularSplitSum and either ambient term.  -1: refused.
extern "C" int bh_light(const crychic_pass_constants* cb, const void* g0, const void* g1, const void* g2,
                        const uint32_t* depth, const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                        const uint8_t* cube, uint32_t cubeDim, uint8_t* out, float* radiance, uint32_t W, uint32_t H,
                        uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                        const crychic_light* pointLights, uint32_t numPointLights, const crychic_light* spotLights,
                        uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim, const uint32_t* const* shadowMaps,
                        uint32_t pointShadowCount, uint32_t pointShadowDim, const uint32_t* const* pointMaps, const float* shadowProj)
{
    using namespace cry;
    if (!(flags & CRYCHIC_LIGHT_ENV_BRDF) || env_brdf_check(flags, cube, cubeDim) != EnvBrdfCheck::Ok ||
        ambient_sh_check(flags, cube, cubeDim) != AmbientShCheck::Ok) return -1;
    return host_light(cb, g0, g1, g2, depth, ambient, shadow, shadowDim, cube, cubeDim, out, radiance, W, H, row0, rows, numDirLights, pcfSearchRadius, flags,
                      pointLights, numPointLights, spotLights, numSpotLights, shadowCount, shadowMapDim, shadowMaps, pointShadowCount,
                      pointShadowDim, pointMaps, shadowProj) ? 0 : -1;
}
