// env_sh_host.cpp -- csrc/cube_sh_core.hpp and the AmbientSH instantiations of light_pixel built for the host (TEST INFRASTRUCTURE):
// the bodies of the kernels of cube_sh.hip and of the SH variants of light_general.hip, bound through light_bind.hpp as the library
// binds them.
#include <cstdint>
#include <cstring>
#include "cube_sh_core.hpp"
#include "../hostsim/host_light.hpp"

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

// Every crychic_deferred_light* entry with CRYCHIC_LIGHT_AMBIENT_SH on the host (tests/hostsim/host_light.hpp): the flag maps onto the
// general family, with AmbientSH and the CubeLevel0 or CubeGloss lookup.  -1: refused.
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
    return host_light(cb, g0, g1, g2, depth, ambient, shadow, shadowDim, cube, cubeDim, out, radiance, W, H, row0, rows, numDirLights, pcfSearchRadius, flags,
                      pointLights, numPointLights, spotLights, numSpotLights, shadowCount, shadowMapDim, shadowMaps, pointShadowCount,
                      pointShadowDim, pointMaps, shadowProj) ? 0 : -1;
}
