// gloss_host.cpp -- csrc/cube_prefilter_core.hpp built for the host (TEST INFRASTRUCTURE): the body of cube_prefilter_kernel, one call
// of cube_prefilter_thread per thread of the launch of a level, whole workgroups of 256 as the launcher sizes the grid.  The tables
// are the product's (crychic_cube_prefilter_samples), handed in by the caller.  And the gloss lighting calls.
#include <cstdint>
#include <cstring>
#include "cube_prefilter_core.hpp"

// tables: levels - 1 records of 32 x 4 floats, a count and 1 / the weight sum (cry::CubePrefilterTable), for levels 1 .. levels - 1
extern "C" void gh_prefilter(const uint8_t* src, uint8_t* dst, uint32_t dim, uint32_t levels, const cry::CubePrefilterTable* tables)
{
    using namespace cry;
    std::memcpy(dst, src, (size_t)6u * dim * dim * 4u);
    uint32_t* level = reinterpret_cast<uint32_t*>(dst);
    for (uint32_t k = 1; k < levels; ++k) {
        const uint32_t dPrev = cube_level_dim(dim, k - 1u), d = cube_level_dim(dim, k);
        level += (size_t)6u * dPrev * dPrev;
        const uint32_t blocks = (6u * d * d + kCubePrefilterThreads - 1u) / kCubePrefilterThreads;
        for (uint32_t idx = 0; idx < blocks * kCubePrefilterThreads; ++idx)
            cube_prefilter_thread(reinterpret_cast<const uint32_t*>(src), level, dim, levels, d, idx, tables[k - 1u]);
    }
}

#include "../hostsim/host_light.hpp"

// Every crychic_deferred_light* entry with CRYCHIC_LIGHT_CUBE_GLOSS on the host (tests/hostsim/host_light.hpp): the flag maps onto the
// general family, with the CubeGloss lookup.
extern "C" void gh_light(const crychic_pass_constants* cb, const void* g0, const void* g1, const void* g2,
                         const uint32_t* depth, const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                         const uint8_t* cube, uint32_t cubeDim, uint8_t* out, float* radiance, uint32_t W, uint32_t H,
                         uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                         const crychic_light* pointLights, uint32_t numPointLights, const crychic_light* spotLights,
                         uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim, const uint32_t* const* shadowMaps,
                         uint32_t pointShadowCount, uint32_t pointShadowDim, const uint32_t* const* pointMaps, const float* shadowProj)
{
    cry::host_light(cb, g0, g1, g2, depth, ambient, shadow, shadowDim, cube, cubeDim, out, radiance, W, H, row0, rows, numDirLights, pcfSearchRadius, flags,
                           pointLights, numPointLights, spotLights, numSpotLights, shadowCount, shadowMapDim, shadowMaps, pointShadowCount,
                           pointShadowDim, pointMaps, shadowProj);
}
