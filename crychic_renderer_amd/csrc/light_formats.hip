// light_formats.hip -- the deferred lighting kernels over G-buffer planes of any format mix (crychic_hip.h CRYCHIC_GBUFFER_G*_F16,
// DESIGN.md section 13): light_tiles.hpp's bodies built over `const void*` planes, where each plane's format is a scalar branch on
// a bit of P.flags at the load (light_core.hpp gbuffer_load).  Eight instantiations serve every light set; launch_light
// (kernels.hip) comes here only when a format bit is set.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.hpp"
#include "light_core.hpp"
#include "light_tiles.hpp"

namespace cry {

// The same pass over planes of any format mix (a CRYCHIC_GBUFFER_G*_F16 bit is set) for frames without local lights.  FIX is
// compiled in, as in the chain's instantiations: this is never the benchmark's kernel.
template <bool ZERO_RADIUS, bool MIPS>
__global__ __launch_bounds__(256) void light_formats_kernel(LightParams P, const void* __restrict__ g0,
                                                            const void* __restrict__ g1, const void* __restrict__ g2,
                                                            const uint32_t* __restrict__ depth,
                                                            const uint16_t* __restrict__ ambient,
                                                            const uint32_t* __restrict__ cube, uint32_t* __restrict__ out,
                                                            f4a* __restrict__ radiance, uint32_t row0, uint32_t row1)
{
    light_frame_tile<ZERO_RADIUS, true, MIPS>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1);
}

// The same kernel over planes of any format mix, for every frame with local lights of whatever kind: counts of 0 are settled at run
// time as above (no spot lights: an empty mask; no shadows: factor 1, the unshadowed bits), so it is the matching entry bit for bit.
template <bool ZERO_RADIUS, bool MIPS>
__global__ __launch_bounds__(256) void light_point_shadows_formats_kernel(LightParams P, const void* __restrict__ g0, const void* __restrict__ g1,
                                                                          const void* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                                          const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                                          uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                                          uint32_t row1, const crychic_light* __restrict__ spots, uint32_t numSpots,
                                                                          SpotShadows shadows, PointShadows pointShadows)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    __shared__ uint32_t s_spotMask[kMaxSpotLights / 32];
    light_local_tile<ZERO_RADIUS, MIPS, true, true, true>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1, s_box, s_mask,
                                                          spots, numSpots, s_spotMask, &shadows, &pointShadows);
}
static_assert(sizeof(LightParams) + sizeof(SpotShadows) + sizeof(PointShadows) + 9 * sizeof(void*) + 3 * sizeof(uint32_t) <= 4096,
              "light_point_shadows_formats_kernel's arguments exceed 4 KiB");

hipError_t launch_light_formats(const LightParams& P, const void* g0, const void* g1, const void* g2, const uint32_t* depth,
                                const uint16_t* ambient, const uint8_t* cube, uint8_t* out, float* radiance, uint32_t row0, uint32_t rows,
                                hipStream_t stream, const crychic_light* spots, uint32_t numSpots, const SpotShadows* shadows,
                                const PointShadows* pointShadows)
{
    if (rows == 0) return hipSuccess;
    const dim3 grid = grid_for(P.W, rows);
    const bool mips = P.cubeLevels > 1u;          // quads inside wavefronts (light_tile_pixel): the rows must start a quad
    if (mips && (row0 & 1u)) return hipErrorInvalidValue;
    auto launch = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, P, g0, g1, g2, depth, ambient, (const uint32_t*)cube, (uint32_t*)out,
                           (f4a*)radiance, row0, row0 + rows, extra...);
    };
    // dispatch(family) calls family(z, m) once: z = <ZERO_RADIUS>, m = <MIPS>, as std::bool_constant
    auto dispatch = [&](auto family) {
        if (P.pcfSearchRadius == 0.0f) { if (mips) family(std::true_type{}, std::true_type{}); else family(std::true_type{}, std::false_type{}); }
        else { if (mips) family(std::false_type{}, std::true_type{}); else family(std::false_type{}, std::false_type{}); }
        return hipGetLastError();
    };
    if (P.numPointLights || numSpots)
        return dispatch([&](auto z, auto m) { launch(light_point_shadows_formats_kernel<z, m>, spots, numSpots, shadows ? *shadows : SpotShadows{},
                                                     pointShadows ? *pointShadows : PointShadows{}); });
    return dispatch([&](auto z, auto m) { launch(light_formats_kernel<z, m>); });
}

}  // namespace cry
