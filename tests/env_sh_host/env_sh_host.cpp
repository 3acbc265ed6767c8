// env_sh_host.cpp -- csrc/cube_sh_core.hpp and the AmbientSH instantiations of light_pixel built for the host (TEST INFRASTRUCTURE):
// the bodies of the kernels of cube_sh.hip and light_env.hip, bound through light_bind.hpp as the library binds them.
#include <cstdint>
#include <cstring>
#include <type_traits>
#include "cube_sh_core.hpp"
#include "light_bind.hpp"

// The body's 28 sums over the texels with index in [first, last) of the level, texel after texel through cube_sh_accumulate.
extern "C" void eh_sums(const uint8_t* level, uint32_t d, uint32_t first, uint32_t last, int64_t* sums)
{
    using namespace cry;
    int64_t s[kCubeShSums] = {};
    for (uint32_t i = first; i < last; ++i) cube_sh_accumulate(reinterpret_cast<const uint32_t*>(level), d, i, s);
    std::memcpy(sums, s, sizeof s);
}

// The accumulate launch as the device runs it -- `blocks` workgroups of 256 lanes, each lane its grid-stride texels, the lanes'
// sums added per workgroup and the workgroups' into the tail's accumulators (any grouping gives the same integers) -- and the
// finalise launch: 36 lanes write the coefficient block.  tail: CRYCHIC_CUBE_SH_BYTES bytes of whatever.
extern "C" void eh_project(const uint8_t* level, uint32_t d, uint8_t* tail, uint32_t blocks)
{
    using namespace cry;
    int64_t sums[kCubeShSums];
    for (uint32_t k = 0; k < kCubeShSums; ++k) sums[k] = 0;                    // the zero launch
    const uint32_t texels = 6u * d * d, stride = blocks * kCubeShThreads;
    for (uint32_t b = 0; b < blocks; ++b) {
        int64_t group[kCubeShSums] = {};
        for (uint32_t t = 0; t < kCubeShThreads; ++t) {
            int64_t lane[kCubeShSums] = {};
            for (uint32_t i = b * kCubeShThreads + t; i < texels; i += stride) cube_sh_accumulate(reinterpret_cast<const uint32_t*>(level), d, i, lane);
            for (uint32_t k = 0; k < kCubeShSums; ++k) group[k] += lane[k];
        }
        for (uint32_t k = 0; k < kCubeShSums; ++k) sums[k] += group[k];
    }
    std::memcpy(tail + kCubeShCoeffBytes, sums, sizeof sums);
    float coeffs[36];
    for (uint32_t i = 0; i < 36u; ++i) coeffs[i] = cube_sh_coefficient(sums, i);
    std::memcpy(tail, coeffs, sizeof coeffs);
}

extern "C" uint64_t eh_tail_offset(uint32_t dim, uint32_t levels) { return cry::ambient_sh_offset(dim, levels); }

// The binding's validation of a call with the flag: 0 ok, 1 derivative-LOD chain, 2 null cube map, 3 misaligned tail.
extern "C" int eh_check(uint32_t flags, uintptr_t cube, uint32_t cubeDim)
{
    return (int)cry::ambient_sh_check(flags, reinterpret_cast<const void*>(cube), cubeDim);
}

// Every crychic_deferred_light* entry with CRYCHIC_LIGHT_AMBIENT_SH on the host, as tests/gloss_host's gh_light runs the gloss calls:
// the family picked by light_family() (the flag maps onto the format-aware families), each pixel of rows [row0, row0 + rows) through
// light_pixel with AmbientSH and the lookup the kernels of light_env.hip instantiate (CubeLevel0 or CubeGloss).  -1: refused.
extern "C" int eh_light(const crychic_pass_constants* cb, const void* g0, const void* g1, const void* g2,
                        const uint32_t* depth, const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                        const uint8_t* cube, uint32_t cubeDim, uint8_t* out, float* radiance, uint32_t W, uint32_t H,
                        uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                        const crychic_light* pointLights, uint32_t numPointLights, const crychic_light* spotLights,
                        uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim, const uint32_t* const* shadowMaps,
                        uint32_t pointShadowCount, uint32_t pointShadowDim, const uint32_t* const* pointMaps, const float* shadowProj)
{
    using namespace cry;
    if (!(flags & CRYCHIC_LIGHT_AMBIENT_SH) || ambient_sh_check(flags, cube, cubeDim) != AmbientShCheck::Ok) return -1;
    LightParams P;
    SpotShadows S;
    PointShadows PS;
    bind_light_params(P, *cb, shadow, shadowDim, cubeDim, W, H, numDirLights, pcfSearchRadius, flags);
    bind_point_lights(P, pointLights, numPointLights);
    bind_spot_shadows(S, *cb, shadowMaps, shadowCount, shadowMapDim);
    bind_point_shadows(PS, pointMaps, shadowProj, pointShadowCount, pointShadowDim);
    const LightFamily family = light_family(P.flags, P.numPointLights, numSpotLights, S.count, PS.count, P.cubeLevels);
    if (family != LightFamily::FormatsFrame && family != LightFamily::FormatsLocal) return -1;
    const bool zero = pcfSearchRadius == 0.0f, gloss = (flags & CRYCHIC_LIGHT_CUBE_GLOSS) != 0;
    const AllLocalLights ll{ pointLights, numPointLights, spotLights, numSpotLights, light_family_spot_shadows(family) ? &S : nullptr,
                             light_family_point_shadows(family) ? &PS : nullptr };
    const uint32_t h0 = flags & CRYCHIC_GBUFFER_G0_F16, h1 = flags & CRYCHIC_GBUFFER_G1_F16, h2 = flags & CRYCHIC_GBUFFER_G2_F16;
    const uint32_t* cubeTexels = (const uint32_t*)cube;
    const AmbientSH sh{ reinterpret_cast<const float*>(cube + ambient_sh_offset(P.cubeDim, P.cubeLevels)) };
    for (uint32_t y = row0; y < row0 + rows; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t idx = y * W + x;
            f4 lit;
            if ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu) {
                const f4a G0 = gbuffer_load(g0, idx, h0), G1 = gbuffer_load(g1, idx, h1), G2 = gbuffer_load(g2, idx, h2);
                auto pixel = [&](auto lights, auto z) {
                    if (gloss) return light_pixel<z, decltype(lights), true, CubeGloss, AmbientSH>(P, G0, G1, G2, ambient, cubeTexels, lights, cube_gloss(P, G1.w), sh);
                    return light_pixel<z, decltype(lights), true, CubeLevel0, AmbientSH>(P, G0, G1, G2, ambient, cubeTexels, lights, CubeLevel0(), sh);
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
