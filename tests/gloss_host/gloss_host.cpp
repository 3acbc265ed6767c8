// gloss_host.cpp -- csrc/cube_prefilter_core.hpp built for the host (TEST INFRASTRUCTURE): the body of cube_prefilter_kernel, one call
// of cube_prefilter_thread per thread of the launch of a level, whole workgroups of 256 as the launcher sizes the grid.  The tables
// are the product's (crychic_cube_prefilter_samples), handed in by the caller.
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

#include <type_traits>
#include "light_bind.hpp"

// Every crychic_deferred_light* entry with CRYCHIC_LIGHT_CUBE_GLOSS on the host, as tests/hostsim's hs_light runs the others: the
// arguments bound through the library's light_bind.hpp, the family picked by its light_family() (the flag maps onto the format-aware
// families: FIX compiled in, both shadow functors for a call with local lights), and each pixel of rows [row0, row0 + rows) through
// light_pixel with the CubeGloss lookup the kernels of light_gloss.hip instantiate.  The sky reads level 0.
extern "C" void gh_light(const crychic_pass_constants* cb, const void* g0, const void* g1, const void* g2,
                         const uint32_t* depth, const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                         const uint8_t* cube, uint32_t cubeDim, uint8_t* out, float* radiance, uint32_t W, uint32_t H,
                         uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                         const crychic_light* pointLights, uint32_t numPointLights, const crychic_light* spotLights,
                         uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim, const uint32_t* const* shadowMaps,
                         uint32_t pointShadowCount, uint32_t pointShadowDim, const uint32_t* const* pointMaps, const float* shadowProj)
{
    using namespace cry;
    LightParams P;
    SpotShadows S;
    PointShadows PS;
    bind_light_params(P, *cb, shadow, shadowDim, cubeDim, W, H, numDirLights, pcfSearchRadius, flags);
    bind_point_lights(P, pointLights, numPointLights);
    bind_spot_shadows(S, *cb, shadowMaps, shadowCount, shadowMapDim);
    bind_point_shadows(PS, pointMaps, shadowProj, pointShadowCount, pointShadowDim);
    const LightFamily family = light_family(P.flags, P.numPointLights, numSpotLights, S.count, PS.count, P.cubeLevels);
    const bool zero = pcfSearchRadius == 0.0f;
    const AllLocalLights ll{ pointLights, numPointLights, spotLights, numSpotLights, light_family_spot_shadows(family) ? &S : nullptr,
                             light_family_point_shadows(family) ? &PS : nullptr };
    const uint32_t h0 = flags & CRYCHIC_GBUFFER_G0_F16, h1 = flags & CRYCHIC_GBUFFER_G1_F16, h2 = flags & CRYCHIC_GBUFFER_G2_F16;
    const uint32_t* cubeTexels = (const uint32_t*)cube;
    for (uint32_t y = row0; y < row0 + rows; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t idx = y * W + x;
            f4 lit;
            if ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu) {
                const f4a G0 = gbuffer_load(g0, idx, h0), G1 = gbuffer_load(g1, idx, h1), G2 = gbuffer_load(g2, idx, h2);
                const CubeGloss cg = cube_gloss(P, G1.w);
                auto pixel = [&](auto lights) {
                    return zero ? light_pixel<true, decltype(lights), true, CubeGloss>(P, G0, G1, G2, ambient, cubeTexels, lights, cg)
                                : light_pixel<false, decltype(lights), true, CubeGloss>(P, G0, G1, G2, ambient, cubeTexels, lights, cg);
                };
                lit = light_family_local(family) ? pixel(ll) : pixel(NoPointLights());
            }
            else if (flags & CRYCHIC_LIGHT_SKY) lit = sky_pixel(P, cubeTexels, x, y);
            else lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
            if (radiance) { radiance[4 * idx] = lit.x; radiance[4 * idx + 1] = lit.y; radiance[4 * idx + 2] = lit.z; radiance[4 * idx + 3] = lit.w; }
            ((uint32_t*)out)[idx] = pack_rgba8(lit);
        }
}
