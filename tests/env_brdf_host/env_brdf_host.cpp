// env_brdf_host.cpp -- csrc/env_brdf_core.hpp and the SpecularSplitSum instantiations of light_pixel built for the host (TEST
// INFRASTRUCTURE): the bodies of the kernels of env_brdf.hip and light_spec.hip, bound through light_bind.hpp as the library binds them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include "env_brdf_core.hpp"
#include "light_bind.hpp"

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

// Every crychic_deferred_light* entry with CRYCHIC_LIGHT_ENV_BRDF on the host, as tests/env_sh_host's eh_light runs the SH calls: the
// family picked by light_family() (the flag maps onto the format-aware families), each pixel of rows [row0, row0 + rows) through
// light_pixel with CubeGloss, SpecularSplitSum and the ambient term the kernels of light_spec.hip instantiate.  -1: refused.
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
    LightParams P;
    SpotShadows S;
    PointShadows PS;
    bind_light_params(P, *cb, shadow, shadowDim, cubeDim, W, H, numDirLights, pcfSearchRadius, flags);
    bind_point_lights(P, pointLights, numPointLights);
    bind_spot_shadows(S, *cb, shadowMaps, shadowCount, shadowMapDim);
    bind_point_shadows(PS, pointMaps, shadowProj, pointShadowCount, pointShadowDim);
    const LightFamily family = light_family(P.flags, P.numPointLights, numSpotLights, S.count, PS.count, P.cubeLevels);
    if (family != LightFamily::FormatsFrame && family != LightFamily::FormatsLocal) return -1;
    const bool zero = pcfSearchRadius == 0.0f, shAmbient = (flags & CRYCHIC_LIGHT_AMBIENT_SH) != 0;
    const AllLocalLights ll{ pointLights, numPointLights, spotLights, numSpotLights, light_family_spot_shadows(family) ? &S : nullptr,
                             light_family_point_shadows(family) ? &PS : nullptr };
    const uint32_t h0 = flags & CRYCHIC_GBUFFER_G0_F16, h1 = flags & CRYCHIC_GBUFFER_G1_F16, h2 = flags & CRYCHIC_GBUFFER_G2_F16;
    const uint32_t* cubeTexels = (const uint32_t*)cube;
    const size_t tableOffset = env_brdf_offset(P.cubeDim, P.cubeLevels);
    const AmbientSH sh{ reinterpret_cast<const float*>(cube + (tableOffset - CRYCHIC_CUBE_SH_BYTES)) };
    const SpecularSplitSum spec{ reinterpret_cast<const uint32_t*>(cube + tableOffset) };
    for (uint32_t y = row0; y < row0 + rows; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t idx = y * W + x;
            f4 lit;
            if ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu) {
                const f4a G0 = gbuffer_load(g0, idx, h0), G1 = gbuffer_load(g1, idx, h1), G2 = gbuffer_load(g2, idx, h2);
                auto pixel = [&](auto lights, auto z) {
                    if (shAmbient) return light_pixel<z, decltype(lights), true, CubeGloss, AmbientSH, SpecularSplitSum>(P, G0, G1, G2, ambient, cubeTexels, lights, cube_gloss(P, G1.w), sh, spec);
                    return light_pixel<z, decltype(lights), true, CubeGloss, AmbientConst, SpecularSplitSum>(P, G0, G1, G2, ambient, cubeTexels, lights, cube_gloss(P, G1.w), AmbientConst(), spec);
                };
                auto by_radius = [&](auto lights) { return zero ? pixel(lights, std::true_type{}) : pixel(lights, std::false_type{}); };
                lit = light_family_local(family) ? by_radius(ll) : by_radius(NoPointLights());
            }
            else if (flags & CRYCHIC_LIGHT_SKY) lit = sky_pixel(P, cubeTexels, x, y);
            else lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
            if (radiance) { radiance[4 * idx] = lit.x; radiance[4 * idx + 1] = lit.y; radiance[4 * idx + 2] = lit.z; radiance[4 * idx + 3] = lit.w; }
            ((uint32_t*)out)[idx] = pack_rgba8(lit);
        }
    return 0;
}
