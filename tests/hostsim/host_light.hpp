// host_light.hpp -- TEST HARNESS ONLY.  One crychic_deferred_light* call on the host, for every harness that runs one (hs_light,
// gh_light, eh_light, bh_light): the arguments bound through the library's own light_bind.hpp, the kernel family picked by its
// light_family() and the instantiation by its light_variant(), and each pixel of rows [row0, row0 + rows) through the light_pixel
// that kernel runs.  g0 / g1 / g2: float4 or half4 texels by the CRYCHIC_GBUFFER_G*_F16 bits of flags (gbuffer_load; no bit: the
// plain f4a load).  The local families iterate every light un-culled (AllLocalLights): the tiled kernels walk the culled lights in
// the same ascending order.  tileMasks != nullptr is the tiled mode: the frame is cut into the kernels' 64 x 4 tiles anchored at row0
// (the same footprint for CubeChain), each tile's box and admitted lights come from light_core.hpp's tile_box_* / tile_light_touches
// -- the very functions light_local_tile calls -- and each pixel walks its tile's admitted lights only, points then spots, ascending
// (TiledLocalLights).  tileMasks receives, per tile in row-major order, the 32 words of the point lights' mask and then the 32 of the
// spot lights'.  A family's kernels carry a shadow functor or they do not, whatever the counts -- light_point_shadows_kernel
// takes the spot lights with SpotShadowOf even at a spot shadow count of 0 (factor 1) -- and the descriptors handed to
// AllLocalLights are non-null exactly for the functors the family compiles in.  The environment terms are read where the kernels
// read them: light_variant_tail's offset behind the cube map.  The sky reads level 0 unless the lookup is the derivative chain.
// Returns false, with nothing written, for a variant no kernel exists for.
#pragma once
#include <cstdint>
#include <cstring>
#include <type_traits>
#include "light_core.hpp"
#include "light_bind.hpp"

namespace cry {

constexpr uint32_t kTileMaskWords = kMaxPointLights / 32 + kMaxSpotLights / 32;     // per tile: point words, then spot words

// AllLocalLights restricted to the lights whose bit is set in the tile's masks: light_local_tile's walk.
struct TiledLocalLights {
    AllLocalLights all;
    const uint32_t* pointMask;
    const uint32_t* spotMask;
    void operator()(f3 pos, f3 albedo, float roughness, float metalness, f3 normal, f3 view, f3& result, bool fixQ3, bool fixQ4) const
    {
        for (uint32_t i = 0; i < all.nPoints; ++i) {
            if (!((pointMask[i >> 5] >> (i & 31u)) & 1u)) continue;
            if (all.pointShadows) pbr_point_light(all.points[i], pos, albedo, roughness, metalness, normal, view, result, fixQ3, fixQ4,
                                                  PointShadowOf{ all.pointShadows, pos, &all.points[i], i });
            else pbr_point_light(all.points[i], pos, albedo, roughness, metalness, normal, view, result, fixQ3, fixQ4);
        }
        for (uint32_t i = 0; i < all.nSpots; ++i) {
            if (!((spotMask[i >> 5] >> (i & 31u)) & 1u)) continue;
            if (all.shadows) pbr_spot_light(all.spots[i], pos, albedo, roughness, metalness, normal, view, result, fixQ3, fixQ4, SpotShadowOf{ all.shadows, pos, i });
            else pbr_spot_light(all.spots[i], pos, albedo, roughness, metalness, normal, view, result, fixQ3, fixQ4);
        }
    }
};

inline bool host_light(const crychic_pass_constants* cb, const void* g0, const void* g1, const void* g2, const uint32_t* depth,
                       const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim, const uint8_t* cube, uint32_t cubeDim,
                       uint8_t* out, float* radiance, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, int numDirLights,
                       float pcfSearchRadius, uint32_t flags, const crychic_light* pointLights, uint32_t numPointLights,
                       const crychic_light* spotLights, uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim,
                       const uint32_t* const* shadowMaps, uint32_t pointShadowCount, uint32_t pointShadowDim, const uint32_t* const* pointMaps,
                       const float* shadowProj, uint32_t* tileMasks = nullptr)
{
    LightParams P;
    SpotShadows S;
    PointShadows PS;
    bind_light_params(P, *cb, shadow, shadowDim, cubeDim, W, H, numDirLights, pcfSearchRadius, flags);
    bind_point_lights(P, pointLights, numPointLights);
    bind_spot_shadows(S, *cb, shadowMaps, shadowCount, shadowMapDim);
    bind_point_shadows(PS, pointMaps, shadowProj, pointShadowCount, pointShadowDim);
    const LightFamily family = light_family(P.flags, P.numPointLights, numSpotLights, S.count, PS.count, P.cubeLevels);
    const LightVariant variant = light_variant(P.flags, P.cubeLevels);
    const bool zero = pcfSearchRadius == 0.0f;
    const AllLocalLights ll{ pointLights, numPointLights, spotLights, numSpotLights, light_family_spot_shadows(family) ? &S : nullptr,
                             light_family_point_shadows(family) ? &PS : nullptr };
    const uint32_t h0 = flags & CRYCHIC_GBUFFER_G0_F16, h1 = flags & CRYCHIC_GBUFFER_G1_F16, h2 = flags & CRYCHIC_GBUFFER_G2_F16;
    auto shaded = [&](uint32_t xx, uint32_t yy) { return xx < W && yy < row0 + rows && (depth[yy * W + xx] & 0x00FFFFFFu) < 0x00FFFFFFu; };
    auto reflection = [&](uint32_t xx, uint32_t yy) { return reflection_dir(P, gbuffer_load(g0, yy * W + xx, h0), gbuffer_load(g2, yy * W + xx, h2)); };
    const uint32_t* cubeTexels = (const uint32_t*)cube;
    // the tiled mode: steps 1 and 2 of light_local_tile for every tile
    const uint32_t tilesX = (W + 63u) / 64u, tilesY = (rows + 3u) / 4u;
    const bool tiled = tileMasks && light_family_local(family);
    if (tileMasks) std::memset(tileMasks, 0, sizeof(uint32_t) * kTileMaskWords * tilesX * tilesY);
    for (uint32_t t = 0; tiled && t < tilesX * tilesY; ++t) {
        TileBox box = tile_box_pixel(false, f4a{ 0, 0, 0, 0 });
        for (uint32_t k = 0; k < 256u; ++k) {
            const uint32_t x = (t % tilesX) * 64u + (k & 63u), y = row0 + (t / tilesX) * 4u + (k >> 6);
            const bool covered = shaded(x, y);
            box = tile_box_merge(box, tile_box_pixel(covered, covered ? gbuffer_load(g0, y * W + x, h0) : f4a{ 0, 0, 0, 0 }));
        }
        if (!tile_box_any_covered(box)) continue;
        uint32_t* m = tileMasks + (size_t)t * kTileMaskWords;
        for (uint32_t l = 0; l < numPointLights; ++l) if (tile_light_touches(pointLights[l], box)) m[l >> 5] |= 1u << (l & 31u);
        for (uint32_t l = 0; l < numSpotLights; ++l) if (tile_light_touches(spotLights[l], box)) m[kMaxPointLights / 32 + (l >> 5)] |= 1u << (l & 31u);
    }
    const size_t tail = light_variant_tail(variant, P.cubeDim, P.cubeLevels);
    const AmbientSH sh{ reinterpret_cast<const float*>(cube + (variant.splitSum ? tail - CRYCHIC_CUBE_SH_BYTES : tail)) };
    const SpecularSplitSum splitSum{ reinterpret_cast<const uint32_t*>(cube + tail) };
    return light_variant_visit(variant, [&](auto cubeTag, auto ambientTag, auto specTag) {
        using Cube = decltype(cubeTag);
        using Ambient = decltype(ambientTag);
        using Specular = decltype(specTag);
        constexpr bool chain = std::is_same_v<Cube, CubeChain>;
        Ambient ambientTerm;
        Specular specTerm;
        if constexpr (Ambient::kSH) ambientTerm = sh;
        if constexpr (Specular::kSplitSum) specTerm = splitSum;
        for (uint32_t y = row0; y < row0 + rows; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                const uint32_t idx = y * W + x;
                f4 lit;
                if (shaded(x, y)) {
                    const f4a G0 = gbuffer_load(g0, idx, h0), G1 = gbuffer_load(g1, idx, h1), G2 = gbuffer_load(g2, idx, h2);
                    float lod = 0.0f;
                    if (chain) {    // the quad neighbours' reflection vectors arrive by lane exchange in the kernels, by recomputation here
                        const f3 r = reflection_dir(P, G0, G2);
                        f3 ddx{ 0.0f, 0.0f, 0.0f }, ddy{ 0.0f, 0.0f, 0.0f };
                        if (shaded(x ^ 1u, y)) { const f3 n = reflection(x ^ 1u, y); ddx = (x & 1u) ? f3{ r.x - n.x, r.y - n.y, r.z - n.z } : f3{ n.x - r.x, n.y - r.y, n.z - r.z }; }
                        if (shaded(x, y ^ 1u)) { const f3 n = reflection(x, y ^ 1u); ddy = (y & 1u) ? f3{ r.x - n.x, r.y - n.y, r.z - n.z } : f3{ n.x - r.x, n.y - r.y, n.z - r.z }; }
                        lod = cube_lod(P.cubeDim, P.cubeLevels, r, ddx, ddy);
                    }
                    const Cube lookup = lookup_for<Cube>(P, G1.w, lod);
                    auto pixel = [&](auto fix, auto lights) {
                        return zero ? light_pixel<true, decltype(lights), decltype(fix)::value, Cube, Ambient, Specular>(P, G0, G1, G2, ambient, cubeTexels, lights, lookup, ambientTerm, specTerm)
                                    : light_pixel<false, decltype(lights), decltype(fix)::value, Cube, Ambient, Specular>(P, G0, G1, G2, ambient, cubeTexels, lights, lookup, ambientTerm, specTerm);
                    };
                    if (tiled) {
                        const uint32_t* m = tileMasks + (size_t)(((y - row0) / 4u) * tilesX + x / 64u) * kTileMaskWords;
                        lit = pixel(std::true_type{}, TiledLocalLights{ ll, m, m + kMaxPointLights / 32 });
                    }
                    else if (light_family_local(family)) lit = pixel(std::true_type{}, ll);      // every local family compiles FIX in
                    else if (light_family_fix(family)) lit = pixel(std::true_type{}, NoPointLights());
                    else lit = pixel(std::false_type{}, NoPointLights());
                }
                else if (flags & CRYCHIC_LIGHT_SKY) lit = chain ? sky_pixel_chain(P, cubeTexels, x, y) : sky_pixel(P, cubeTexels, x, y);
                else lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
                if (radiance) { radiance[4 * idx] = lit.x; radiance[4 * idx + 1] = lit.y; radiance[4 * idx + 2] = lit.z; radiance[4 * idx + 3] = lit.w; }
                ((uint32_t*)out)[idx] = pack_rgba8(lit);
            }
    });
}

}  // namespace cry
