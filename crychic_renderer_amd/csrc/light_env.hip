// light_env.hip -- the deferred lighting kernels with the ambient term from the environment (crychic_hip.h CRYCHIC_LIGHT_AMBIENT_SH,
// DESIGN.md section 16): light_tiles.hpp's bodies with AmbientSH, where the colour of DeferredShading.hlsl:44 is the SH9 irradiance
// along the pixel's normal, from the coefficient block that follows the cube map at cube + shOffset bytes.  As the gloss kernels do,
// every call maps onto the most general family of its shape: planes of any format mix (no format bit: float4), FIX compiled in,
// and for a call with local lights both shadow functors whatever the counts.  The lookup is level 0 alone (no chain) or CubeGloss
// (a prefiltered chain); the derivative-LOD chain is refused by the entries.  Eight instantiations; launch_light (kernels.hip) comes
// here only when the flag is set, so no other kernel changes.  shOffset is an argument of these kernels alone: LightParams keeps
// its layout.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.hpp"
#include "light_core.hpp"
#include "light_tiles.hpp"
#include "light_bind.hpp"

namespace cry {

// wave-uniform: two kernel arguments added
__device__ __forceinline__ AmbientSH ambient_sh_at(const uint32_t* __restrict__ cube, size_t shOffset)
{
    return AmbientSH{ reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(cube) + shOffset) };
}

template <bool ZERO_RADIUS, bool GLOSS>
__global__ __launch_bounds__(256) void light_env_kernel(LightParams P, const void* __restrict__ g0,
                                                        const void* __restrict__ g1, const void* __restrict__ g2,
                                                        const uint32_t* __restrict__ depth,
                                                        const uint16_t* __restrict__ ambient,
                                                        const uint32_t* __restrict__ cube, uint32_t* __restrict__ out,
                                                        f4a* __restrict__ radiance, uint32_t row0, uint32_t row1, size_t shOffset)
{
    light_frame_tile<ZERO_RADIUS, true, false, void, GLOSS, AmbientSH>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1,
                                                                       ambient_sh_at(cube, shOffset));
}

// Every such frame with local lights of whatever kind: counts of 0 are settled at run time.
template <bool ZERO_RADIUS, bool GLOSS>
__global__ __launch_bounds__(256) void light_env_local_kernel(LightParams P, const void* __restrict__ g0, const void* __restrict__ g1,
                                                              const void* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                              const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                              uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                              uint32_t row1, size_t shOffset, const crychic_light* __restrict__ spots,
                                                              uint32_t numSpots, SpotShadows shadows, PointShadows pointShadows)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    __shared__ uint32_t s_spotMask[kMaxSpotLights / 32];
    light_local_tile<ZERO_RADIUS, false, true, true, true, void, GLOSS, AmbientSH>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1,
                                                                                   s_box, s_mask, spots, numSpots, s_spotMask, &shadows,
                                                                                   &pointShadows, ambient_sh_at(cube, shOffset));
}
static_assert(sizeof(LightParams) + sizeof(SpotShadows) + sizeof(PointShadows) + 10 * sizeof(void*) + 3 * sizeof(uint32_t) <= 4096,
              "light_env_local_kernel's arguments exceed 4 KiB");

hipError_t launch_light_env(const LightParams& P, const void* g0, const void* g1, const void* g2, const uint32_t* depth,
                            const uint16_t* ambient, const uint8_t* cube, uint8_t* out, float* radiance, uint32_t row0, uint32_t rows,
                            hipStream_t stream, const crychic_light* spots, uint32_t numSpots, const SpotShadows* shadows,
                            const PointShadows* pointShadows)
{
    if (rows == 0) return hipSuccess;
    const bool gloss = (P.flags & CRYCHIC_LIGHT_CUBE_GLOSS) != 0;
    if (gloss ? P.cubeLevels < 2u : P.cubeLevels > 1u) return hipErrorInvalidValue;     // api.cpp reports both
    const size_t shOffset = ambient_sh_offset(P.cubeDim, P.cubeLevels);
    if ((reinterpret_cast<uintptr_t>(cube) + shOffset) & 3u) return hipErrorInvalidValue;
    const dim3 grid = grid_for(P.W, rows);
    auto launch = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, P, g0, g1, g2, depth, ambient, (const uint32_t*)cube, (uint32_t*)out,
                           (f4a*)radiance, row0, row0 + rows, shOffset, extra...);
    };
    auto by_shape = [&](auto family) {
        if (P.pcfSearchRadius == 0.0f) { if (gloss) family(std::true_type{}, std::true_type{}); else family(std::true_type{}, std::false_type{}); }
        else { if (gloss) family(std::false_type{}, std::true_type{}); else family(std::false_type{}, std::false_type{}); }
        return hipGetLastError();
    };
    if (P.numPointLights || numSpots)
        return by_shape([&](auto z, auto g) { launch(light_env_local_kernel<z, g>, spots, numSpots, shadows ? *shadows : SpotShadows{},
                                                     pointShadows ? *pointShadows : PointShadows{}); });
    return by_shape([&](auto z, auto g) { launch(light_env_kernel<z, g>); });
}

}  // namespace cry
