// host_light_probe.hpp -- TEST HARNESS ONLY.  tests/hostsim/host_light.hpp's lighting call for a variant with the box-projected
// reflection lookup (CRYCHIC_LIGHT_CUBE_PARALLAX): host_light cannot hand the probe volume's address to the lookup, so this is its
// pixel loop with that one difference -- the volume is read where the kernels read it (parallax_probe_offset behind the cube map,
// probe_load) and handed to lookup_for -- through the same light_bind.hpp binding and the variant visit launch_light_general goes
// through (light_variant_visit_all).  No tiled mode and no derivative chain: a parallax variant has neither.  A call without the
// flag goes to host_light itself.  Returns false, with nothing written, for a variant no kernel exists for.
#pragma once
#include "../hostsim/host_light.hpp"

namespace cry {

inline bool host_light_probe(const crychic_pass_constants* cb, const void* g0, const void* g1, const void* g2, const uint32_t* depth,
                             const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim, const uint8_t* cube, uint32_t cubeDim,
                             uint8_t* out, float* radiance, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, int numDirLights,
                             float pcfSearchRadius, uint32_t flags, const crychic_light* pointLights, uint32_t numPointLights,
                             const crychic_light* spotLights, uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim,
                             const uint32_t* const* shadowMaps, uint32_t pointShadowCount, uint32_t pointShadowDim, const uint32_t* const* pointMaps,
                             const float* shadowProj)
{
    if (!(flags & CRYCHIC_LIGHT_CUBE_PARALLAX))
        return host_light(cb, g0, g1, g2, depth, ambient, shadow, shadowDim, cube, cubeDim, out, radiance, W, H, row0, rows, numDirLights, pcfSearchRadius,
                          flags, pointLights, numPointLights, spotLights, numSpotLights, shadowCount, shadowMapDim, shadowMaps, pointShadowCount,
                          pointShadowDim, pointMaps, shadowProj);
    LightParams P;
    SpotShadows S;
    PointShadows PS;
    bind_light_params(P, *cb, shadow, shadowDim, cubeDim, W, H, numDirLights, pcfSearchRadius, flags);
    bind_point_lights(P, pointLights, numPointLights);
    bind_spot_shadows(S, *cb, shadowMaps, shadowCount, shadowMapDim);
    bind_point_shadows(PS, pointMaps, shadowProj, pointShadowCount, pointShadowDim);
    const LightFamily family = light_family(P.flags, P.numPointLights, numSpotLights, S.count, PS.count, P.cubeLevels);
    const LightVariant variant = light_variant(P.flags, P.cubeLevels);
    if (!variant.parallax || variant.lookup != CubeLookup::Gloss || P.cubeLevels < 2u) return false;
    const bool zero = pcfSearchRadius == 0.0f;
    const AllLocalLights ll{ pointLights, numPointLights, spotLights, numSpotLights, light_family_spot_shadows(family) ? &S : nullptr,
                             light_family_point_shadows(family) ? &PS : nullptr };
    const uint32_t h0 = flags & CRYCHIC_GBUFFER_G0_F16, h1 = flags & CRYCHIC_GBUFFER_G1_F16, h2 = flags & CRYCHIC_GBUFFER_G2_F16;
    const uint32_t* cubeTexels = (const uint32_t*)cube;
    const size_t tail = light_variant_tail(variant, P.cubeDim, P.cubeLevels);
    const AmbientSH sh{ reinterpret_cast<const float*>(cube + (variant.splitSum ? tail - CRYCHIC_CUBE_SH_BYTES : tail)) };
    const SpecularSplitSum splitSum{ reinterpret_cast<const uint32_t*>(cube + tail) };
    const ProbeVolume probe = probe_load(reinterpret_cast<const float*>(cube + parallax_probe_offset(P.cubeDim, P.cubeLevels)));
    return light_variant_visit_all(variant, [&](auto cubeTag, auto ambientTag, auto specTag) {
        using Cube = decltype(cubeTag);
        using Ambient = decltype(ambientTag);
        using Specular = decltype(specTag);
        Ambient ambientTerm;
        Specular specTerm;
        if constexpr (Ambient::kSH) ambientTerm = sh;
        if constexpr (Specular::kSplitSum) specTerm = splitSum;
        for (uint32_t y = row0; y < row0 + rows; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                const uint32_t idx = y * W + x;
                f4 lit;
                if ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu) {
                    const f4a G0 = gbuffer_load(g0, idx, h0), G1 = gbuffer_load(g1, idx, h1), G2 = gbuffer_load(g2, idx, h2);
                    const Cube lookup = lookup_for<Cube>(P, G1.w, 0.0f, probe);
                    auto pixel = [&](auto lights) {      // the general family compiles FIX in
                        return zero ? light_pixel<true, decltype(lights), true, Cube, Ambient, Specular>(P, G0, G1, G2, ambient, cubeTexels, lights, lookup, ambientTerm, specTerm)
                                    : light_pixel<false, decltype(lights), true, Cube, Ambient, Specular>(P, G0, G1, G2, ambient, cubeTexels, lights, lookup, ambientTerm, specTerm);
                    };
                    if (light_family_local(family)) lit = pixel(ll); else lit = pixel(NoPointLights());
                }
                else if (flags & CRYCHIC_LIGHT_SKY) lit = sky_pixel(P, cubeTexels, x, y);
                else lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
                if (radiance) { radiance[4 * idx] = lit.x; radiance[4 * idx + 1] = lit.y; radiance[4 * idx + 2] = lit.z; radiance[4 * idx + 3] = lit.w; }
                ((uint32_t*)out)[idx] = pack_rgba8(lit);
            }
    });
}

}  // namespace cry
