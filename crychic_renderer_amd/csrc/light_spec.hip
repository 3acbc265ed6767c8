// light_spec.hip -- the deferred lighting kernels with the split-sum weight of the reflection term (crychic_hip.h
// CRYCHIC_LIGHT_ENV_BRDF): light_tiles.hpp's bodies with SpecularSplitSum, where DeferredShading.hlsl:97 becomes
// lit += fma(R0, A, B) * reflection with (A, B) filtered from the 32 x 32 table that follows the environment tail at cube +
// tableOffset bytes.  As the gloss and env kernels do, every call maps onto the most general family of its shape: planes of any
// format mix (no format bit: float4), FIX compiled in, and for a call with local lights both shadow functors whatever the counts.
// The lookup is always CubeGloss (the entries refuse anything else); the ambient term is the constant or AmbientSH, whose block sits
// CRYCHIC_CUBE_SH_BYTES before the table.  Eight instantiations; launch_light (kernels.hip) comes here only when the flag is set, so
// no other kernel changes.  tableOffset is an argument of these kernels alone: LightParams keeps its layout.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.hpp"
#include "light_core.hpp"
#include "light_tiles.hpp"
#include "light_bind.hpp"

namespace cry {

// wave-uniform: two kernel arguments added
__device__ __forceinline__ SpecularSplitSum split_sum_at(const uint32_t* __restrict__ cube, size_t tableOffset)
{
    return SpecularSplitSum{ reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(cube) + tableOffset) };
}
template <class Ambient>
__device__ __forceinline__ Ambient spec_ambient_at(const uint32_t* __restrict__ cube, size_t tableOffset)
{
    if constexpr (Ambient::kSH)
        return AmbientSH{ reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(cube) + (tableOffset - CRYCHIC_CUBE_SH_BYTES)) };
    else
        return AmbientConst{};
}

template <bool ZERO_RADIUS, class Ambient>
__global__ __launch_bounds__(256) void light_spec_kernel(LightParams P, const void* __restrict__ g0,
                                                         const void* __restrict__ g1, const void* __restrict__ g2,
                                                         const uint32_t* __restrict__ depth,
                                                         const uint16_t* __restrict__ ambient,
                                                         const uint32_t* __restrict__ cube, uint32_t* __restrict__ out,
                                                         f4a* __restrict__ radiance, uint32_t row0, uint32_t row1, size_t tableOffset)
{
    light_frame_tile<ZERO_RADIUS, true, false, void, true, Ambient, SpecularSplitSum>(P, g0, g1, g2, depth, ambient, cube, out, radiance,
                                                                                      row0, row1, spec_ambient_at<Ambient>(cube, tableOffset),
                                                                                      split_sum_at(cube, tableOffset));
}

// Every such frame with local lights of whatever kind: counts of 0 are settled at run time.
template <bool ZERO_RADIUS, class Ambient>
__global__ __launch_bounds__(256) void light_spec_local_kernel(LightParams P, const void* __restrict__ g0, const void* __restrict__ g1,
                                                               const void* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                               const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                               uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                               uint32_t row1, size_t tableOffset, const crychic_light* __restrict__ spots,
                                                               uint32_t numSpots, SpotShadows shadows, PointShadows pointShadows)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    __shared__ uint32_t s_spotMask[kMaxSpotLights / 32];
    light_local_tile<ZERO_RADIUS, false, true, true, true, void, true, Ambient, SpecularSplitSum>(
        P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1, s_box, s_mask, spots, numSpots, s_spotMask, &shadows, &pointShadows,
        spec_ambient_at<Ambient>(cube, tableOffset), split_sum_at(cube, tableOffset));
}
static_assert(sizeof(LightParams) + sizeof(SpotShadows) + sizeof(PointShadows) + 10 * sizeof(void*) + 3 * sizeof(uint32_t) <= 4096,
              "light_spec_local_kernel's arguments exceed 4 KiB");

hipError_t launch_light_spec(const LightParams& P, const void* g0, const void* g1, const void* g2, const uint32_t* depth,
                             const uint16_t* ambient, const uint8_t* cube, uint8_t* out, float* radiance, uint32_t row0, uint32_t rows,
                             hipStream_t stream, const crychic_light* spots, uint32_t numSpots, const SpotShadows* shadows,
                             const PointShadows* pointShadows)
{
    if (rows == 0) return hipSuccess;
    if (!(P.flags & CRYCHIC_LIGHT_CUBE_GLOSS) || P.cubeLevels < 2u) return hipErrorInvalidValue;     // api.cpp reports it
    const size_t tableOffset = env_brdf_offset(P.cubeDim, P.cubeLevels);
    if ((reinterpret_cast<uintptr_t>(cube) + tableOffset) & 3u) return hipErrorInvalidValue;
    const bool sh = (P.flags & CRYCHIC_LIGHT_AMBIENT_SH) != 0;
    const dim3 grid = grid_for(P.W, rows);
    auto launch = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, P, g0, g1, g2, depth, ambient, (const uint32_t*)cube, (uint32_t*)out,
                           (f4a*)radiance, row0, row0 + rows, tableOffset, extra...);
    };
    auto by_shape = [&](auto family) {
        if (P.pcfSearchRadius == 0.0f) { if (sh) family(std::true_type{}, AmbientSH{}); else family(std::true_type{}, AmbientConst{}); }
        else { if (sh) family(std::false_type{}, AmbientSH{}); else family(std::false_type{}, AmbientConst{}); }
        return hipGetLastError();
    };
    if (P.numPointLights || numSpots)
        return by_shape([&](auto z, auto a) { launch(light_spec_local_kernel<z, decltype(a)>, spots, numSpots, shadows ? *shadows : SpotShadows{},
                                                     pointShadows ? *pointShadows : PointShadows{}); });
    return by_shape([&](auto z, auto a) { launch(light_spec_kernel<z, decltype(a)>); });
}

}  // namespace cry
