// light_gloss.hip -- the deferred lighting kernels with the glossy reflection lookup (crychic_hip.h CRYCHIC_LIGHT_CUBE_GLOSS, DESIGN.md
// section 15): light_tiles.hpp's bodies with GLOSS, where the reflection reads the prefiltered chain at the level of the pixel's
// roughness (light_core.hpp CubeGloss).  To bound the number of kernels every gloss call maps onto the most general family of its
// shape, as the format-aware kernels of light_formats.hip do: planes of any format mix (no format bit: float4), FIX compiled in, and
// for a call with local lights both shadow functors whatever the counts.  Four instantiations; launch_light (kernels.hip) comes here
// only when the flag is set, so no other kernel changes.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.hpp"
#include "light_core.hpp"
#include "light_tiles.hpp"

namespace cry {

template <bool ZERO_RADIUS>
__global__ __launch_bounds__(256) void light_gloss_kernel(LightParams P, const void* __restrict__ g0,
                                                          const void* __restrict__ g1, const void* __restrict__ g2,
                                                          const uint32_t* __restrict__ depth,
                                                          const uint16_t* __restrict__ ambient,
                                                          const uint32_t* __restrict__ cube, uint32_t* __restrict__ out,
                                                          f4a* __restrict__ radiance, uint32_t row0, uint32_t row1)
{
    light_frame_tile<ZERO_RADIUS, true, false, void, true>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1);
}

// Every gloss frame with local lights of whatever kind: counts of 0 are settled at run time (no spot lights: an empty mask; no
// shadows: factor 1, the unshadowed bits).
template <bool ZERO_RADIUS>
__global__ __launch_bounds__(256) void light_gloss_local_kernel(LightParams P, const void* __restrict__ g0, const void* __restrict__ g1,
                                                                const void* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                                const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                                uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                                uint32_t row1, const crychic_light* __restrict__ spots, uint32_t numSpots,
                                                                SpotShadows shadows, PointShadows pointShadows)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    __shared__ uint32_t s_spotMask[kMaxSpotLights / 32];
    light_local_tile<ZERO_RADIUS, false, true, true, true, void, true>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1, s_box,
                                                                       s_mask, spots, numSpots, s_spotMask, &shadows, &pointShadows);
}
static_assert(sizeof(LightParams) + sizeof(SpotShadows) + sizeof(PointShadows) + 9 * sizeof(void*) + 3 * sizeof(uint32_t) <= 4096,
              "light_gloss_local_kernel's arguments exceed 4 KiB");

hipError_t launch_light_gloss(const LightParams& P, const void* g0, const void* g1, const void* g2, const uint32_t* depth,
                              const uint16_t* ambient, const uint8_t* cube, uint8_t* out, float* radiance, uint32_t row0, uint32_t rows,
                              hipStream_t stream, const crychic_light* spots, uint32_t numSpots, const SpotShadows* shadows,
                              const PointShadows* pointShadows)
{
    if (rows == 0) return hipSuccess;
    if (P.cubeLevels < 2u) return hipErrorInvalidValue;          // the flag needs a chain (api.cpp reports it)
    const dim3 grid = grid_for(P.W, rows);
    auto launch = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, P, g0, g1, g2, depth, ambient, (const uint32_t*)cube, (uint32_t*)out,
                           (f4a*)radiance, row0, row0 + rows, extra...);
    };
    auto by_radius = [&](auto family) {
        if (P.pcfSearchRadius == 0.0f) family(std::true_type{}); else family(std::false_type{});
        return hipGetLastError();
    };
    if (P.numPointLights || numSpots)
        return by_radius([&](auto z) { launch(light_gloss_local_kernel<z>, spots, numSpots, shadows ? *shadows : SpotShadows{},
                                              pointShadows ? *pointShadows : PointShadows{}); });
    return by_radius([&](auto z) { launch(light_gloss_kernel<z>); });
}

}  // namespace cry
