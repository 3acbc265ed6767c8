// light_general.hip -- the general family of the deferred lighting kernels: light_tiles.hpp's bodies over
// `const void*` planes of any format mix (each plane's format is a scalar branch on a bit of P.flags at the load: light_core.hpp
// gbuffer_load; no format bit: float4), FIX compiled in, and for a call with local lights both shadow functors whatever the counts.
// Every call with a CRYCHIC_GBUFFER_G*_F16 bit, CRYCHIC_LIGHT_CUBE_GLOSS (with or without CRYCHIC_LIGHT_CUBE_PARALLAX),
// CRYCHIC_LIGHT_AMBIENT_SH or CRYCHIC_LIGHT_ENV_BRDF comes here (light_bind.hpp light_family), so no kernel of kernels.hip carries a trace of them.  What distinguishes the instantiations is
// the LightVariant of light_bind.hpp: the cube lookup, the ambient term and the weight of the reflection.  Seven variants x
// ZERO_RADIUS x (frame | local) = 28 kernels, and four more variants with the box-projected lookup (CRYCHIC_LIGHT_CUBE_PARALLAX,
// DESIGN.md section 18): 16 kernels.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.hpp"
#include "light_core.hpp"
#include "light_tiles.hpp"
#include "light_bind.hpp"

namespace cry {

// The environment terms of a variant that has any: Tail is one size_t after row1, light_variant_tail's offset behind the cube map
// -- an argument of these kernels alone, so LightParams keeps its layout.  Wave-uniform: two kernel arguments added.
template <class Ambient, class Specular>
__device__ __forceinline__ Ambient ambient_at(const uint32_t* __restrict__ cube, size_t tail = 0)
{
    if constexpr (Ambient::kSH)       // the coefficient block sits CRYCHIC_CUBE_SH_BYTES before the table
        return AmbientSH{ reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(cube) + (Specular::kSplitSum ? tail - CRYCHIC_CUBE_SH_BYTES : tail)) };
    else
        return AmbientConst{};
}
template <class Specular>
__device__ __forceinline__ Specular split_sum_at(const uint32_t* __restrict__ cube, size_t tail = 0)
{
    if constexpr (Specular::kSplitSum)
        return SpecularSplitSum{ reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(cube) + tail) };
    else
        return SpecularRef{};
}

// CubeGlossBox: the probe volume sits CRYCHIC_CUBE_PROBE_OFFSET into the environment tail, which starts where the coefficient block
// does; every box variant takes the Tail argument, whatever its ambient term and weight.
template <class Cube, class Specular>
__device__ __forceinline__ const float* probe_at(const uint32_t* __restrict__ cube, size_t tail = 0)
{
    if constexpr (std::is_same_v<Cube, CubeGlossBox>)
        return reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(cube) + (Specular::kSplitSum ? tail - CRYCHIC_CUBE_SH_BYTES : tail) + CRYCHIC_CUBE_PROBE_OFFSET);
    else
        return nullptr;
}

// A frame without local lights.  Never the benchmark's kernel.
template <bool ZERO_RADIUS, class Cube, class Ambient, class Specular, class... Tail>
__global__ __launch_bounds__(256) void light_general_kernel(LightParams P, const void* __restrict__ g0,
                                                            const void* __restrict__ g1, const void* __restrict__ g2,
                                                            const uint32_t* __restrict__ depth,
                                                            const uint16_t* __restrict__ ambient,
                                                            const uint32_t* __restrict__ cube, uint32_t* __restrict__ out,
                                                            f4a* __restrict__ radiance, uint32_t row0, uint32_t row1, Tail... tail)
{
    light_frame_tile<ZERO_RADIUS, true, Cube, void, Ambient, Specular>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1,
                                                                       ambient_at<Ambient, Specular>(cube, tail...),
                                                                       split_sum_at<Specular>(cube, tail...), probe_at<Cube, Specular>(cube, tail...));
}

// Every frame with local lights of whatever kind: counts of 0 are settled at run time (no spot lights: an empty mask; no shadows:
// factor 1, the unshadowed bits), so it is the matching entry bit for bit.
template <bool ZERO_RADIUS, class Cube, class Ambient, class Specular, class... Tail>
__global__ __launch_bounds__(256) void light_general_local_kernel(LightParams P, const void* __restrict__ g0, const void* __restrict__ g1,
                                                                  const void* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                                  const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                                  uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                                  uint32_t row1, Tail... tail, const crychic_light* __restrict__ spots,
                                                                  uint32_t numSpots, SpotShadows shadows, PointShadows pointShadows)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    __shared__ uint32_t s_spotMask[kMaxSpotLights / 32];
    light_local_tile<ZERO_RADIUS, Cube, true, true, true, void, Ambient, Specular>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1,
                                                                                   s_box, s_mask, spots, numSpots, s_spotMask, &shadows,
                                                                                   &pointShadows, ambient_at<Ambient, Specular>(cube, tail...),
                                                                                   split_sum_at<Specular>(cube, tail...), probe_at<Cube, Specular>(cube, tail...));
}
static_assert(sizeof(LightParams) + sizeof(SpotShadows) + sizeof(PointShadows) + 10 * sizeof(void*) + 3 * sizeof(uint32_t) <= 4096,
              "light_general_local_kernel's arguments exceed 4 KiB");

hipError_t launch_light_general(const LightParams& P, const void* g0, const void* g1, const void* g2, const uint32_t* depth,
                                const uint16_t* ambient, const uint8_t* cube, uint8_t* out, float* radiance, uint32_t row0, uint32_t rows,
                                hipStream_t stream, const crychic_light* spots, uint32_t numSpots, const SpotShadows* shadows,
                                const PointShadows* pointShadows)
{
    if (rows == 0) return hipSuccess;
    const LightVariant v = light_variant(P.flags, P.cubeLevels);
    // api.cpp reports all of these: the gloss lookup needs a chain; the derivative chain has its quads inside wavefronts
    // (light_tile_pixel), so the rows must start one; the environment terms are read as dwords
    if (v.lookup == CubeLookup::Gloss && P.cubeLevels < 2u) return hipErrorInvalidValue;
    if (v.lookup == CubeLookup::DerivativeChain && (row0 & 1u)) return hipErrorInvalidValue;
    const size_t tail = light_variant_tail(v, P.cubeDim, P.cubeLevels);
    if ((v.ambientSH || v.splitSum || v.parallax) && ((reinterpret_cast<uintptr_t>(cube) + tail) & 3u)) return hipErrorInvalidValue;
    const dim3 grid = grid_for(P.W, rows);
    const bool local = P.numPointLights || numSpots;
    // one kernel of <z, Cube, Ambient, Specular, decltype(t)...>: the frame's or the local one, whose own arguments follow the tail
    auto launch = [&](auto z, auto c, auto a, auto s, auto... t) {
        if (local)
            hipLaunchKernelGGL((light_general_local_kernel<z, decltype(c), decltype(a), decltype(s), decltype(t)...>), grid, dim3(256), 0, stream, P,
                               g0, g1, g2, depth, ambient, (const uint32_t*)cube, (uint32_t*)out, (f4a*)radiance, row0, row0 + rows, t..., spots,
                               numSpots, shadows ? *shadows : SpotShadows{}, pointShadows ? *pointShadows : PointShadows{});
        else
            hipLaunchKernelGGL((light_general_kernel<z, decltype(c), decltype(a), decltype(s), decltype(t)...>), grid, dim3(256), 0, stream, P,
                               g0, g1, g2, depth, ambient, (const uint32_t*)cube, (uint32_t*)out, (f4a*)radiance, row0, row0 + rows, t...);
    };
    const bool served = light_variant_visit_all(v, [&](auto c, auto a, auto s) {
        auto by_radius = [&](auto... t) {
            if (P.pcfSearchRadius == 0.0f) launch(std::true_type{}, c, a, s, t...); else launch(std::false_type{}, c, a, s, t...);
        };
        if constexpr (decltype(a)::kSH || decltype(s)::kSplitSum || std::is_same_v<decltype(c), CubeGlossBox>) by_radius(tail); else by_radius();
    });
    return served ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace cry
