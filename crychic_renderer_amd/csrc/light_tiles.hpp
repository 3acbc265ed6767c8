// light_tiles.hpp -- the per-workgroup bodies of the deferred lighting kernels (device code), shared by the float4 kernels of
// kernels.hip and the general family of light_general.hip (planes of any format mix and every flagged lookup, ambient and specular
// term: DESIGN.md section 13).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "light_core.hpp"
#include "dispatch_order.hpp"

namespace cry {

// CRY_GBUFFER_TEXEL(g, idx, isHalf): texel idx of G-buffer plane g, a `const PLANE*` of the enclosing template.  PLANE = f4a (the
// kernels of kernels.hip): g[idx], with no trace of the formats; PLANE = void: float4 or half4 by the caller's bit of P.flags
// (light_core.hpp gbuffer_load).  An expression at the load site on purpose: handing the plane pointer to a helper function moves
// the register allocation of the float4 kernels (the pointer is a __restrict__ kernel argument there), and those kernels have to
// stay exactly what they were (tools/resusage.sh).
#define CRY_GBUFFER_TEXEL(g, idx, isHalf) ([&]() -> f4a { if constexpr (std::is_void_v<PLANE>) return gbuffer_load(g, idx, isHalf); else return g[idx]; }())

// XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2), so with
// the natural order every XCD touches the whole frame: the SSAO depth taps then miss L2 eight times over
// (measured: 362 MB fetched per 4K launch against 50 MB of planes).  The remap hands each XCD stripes of STRIPE
// consecutive tile rows, interleaved over the frame with period 8*STRIPE: neighbouring tiles -- which share tap
// footprints and blur aprons -- share an L2, while cheap (sky) and expensive (near geometry) regions still spread
// over all XCDs (one contiguous band per XCD measured 1.8x SLOWER on the lighting pass: load imbalance).
// Placement is a performance hint only: any dispatch order produces the same pixels.
template <uint32_t STRIPE>
__device__ __forceinline__ void tile_origin(uint32_t& bx, uint32_t& by)
{
    const uint32_t nbx = gridDim.x, n = nbx * gridDim.y;
    uint32_t b = blockIdx.y * nbx + blockIdx.x;
    if (STRIPE > 0) {
        const uint32_t chunk = nbx * STRIPE;              // tiles per stripe
        const uint32_t full = (n / (chunk * 8u)) * (chunk * 8u);   // tiles covered by whole 8-stripe groups
        if (b < full) {
            const uint32_t xcd = b & 7u, k = b >> 3;      // k-th tile this XCD receives
            const uint32_t j = k / chunk, o = k - j * chunk;
            b = (j * 8u + xcd) * chunk + o;
        }                                                 // the tail keeps its ids (bijective)
    }
    by = b / nbx;
    bx = b - by * nbx;
}

// ---- deferred lighting -----------------------------------------------------------------------------------------
// Shaders/DeferredShading.hlsl:23-101 as a full-screen pass over rows [row0, row1), masked by depth < 1.
// Cube, the lookup policy of light_core.hpp (CubeLevel0 / CubeChain / CubeGloss), decides the footprint.  CubeChain (the cube map
// holds a mip chain sampled by derivatives, P.cubeLevels > 1 without CRYCHIC_LIGHT_CUBE_GLOSS): a wavefront covers 32 x 2 pixels
// instead of 64 x 1, so that every 2 x 2 quad of the frame lies inside one wavefront -- the x neighbour is lane ^ 1, the y
// neighbour lane ^ 32 -- and the level of detail of the reflection lookup comes from the neighbours' reflection vectors without a
// second pass (light_core.hpp "TextureCube.Sample with the mip chain bound").  The kernels of kernels.hip spell the choice as
// their MIPS parameter.
template <bool MIPS> using CubeOfMips = std::conditional_t<MIPS, CubeChain, CubeLevel0>;
template <class Cube> constexpr bool kQuads = std::is_same_v<Cube, CubeChain>;
template <bool QUADS>
__device__ __forceinline__ void light_tile_pixel(uint32_t bx, uint32_t by, uint32_t row0, uint32_t& x, uint32_t& y)
{
    if (QUADS) {
        const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
        x = bx * 64u + (wave & 1u) * 32u + (lane & 31u);
        y = row0 + by * 4u + (wave >> 1) * 2u + (lane >> 5);
    } else {
        x = bx * 64u + (threadIdx.x & 63u);
        y = row0 + by * 4u + (threadIdx.x >> 6);
    }
}
// The level of detail of this lane's reflection lookup; every lane of the wavefront calls it (converged).  `r` is the lane's
// reflection vector when `covered`.  A neighbour the pass does not shade contributes a zero derivative (the oracle's definition).
__device__ __forceinline__ float quad_reflection_lod(const LightParams& P, bool covered, f3 r, uint32_t x, uint32_t y)
{
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(covered);
    const uint32_t lane = threadIdx.x & 63u;
    const f3 nx{ __shfl_xor(r.x, 1), __shfl_xor(r.y, 1), __shfl_xor(r.z, 1) };
    const f3 ny{ __shfl_xor(r.x, 32), __shfl_xor(r.y, 32), __shfl_xor(r.z, 32) };
    const bool hasX = (mask >> (lane ^ 1u)) & 1ull, hasY = (mask >> (lane ^ 32u)) & 1ull;
    f3 ddx{ 0.0f, 0.0f, 0.0f }, ddy{ 0.0f, 0.0f, 0.0f };
    if (hasX) ddx = (x & 1u) ? f3{ r.x - nx.x, r.y - nx.y, r.z - nx.z } : f3{ nx.x - r.x, nx.y - r.y, nx.z - r.z };
    if (hasY) ddy = (y & 1u) ? f3{ r.x - ny.x, r.y - ny.y, r.z - ny.z } : f3{ ny.x - r.x, ny.y - r.y, ny.z - r.z };
    return cube_lod(P.cubeDim, P.cubeLevels, r, ddx, ddy);
}

// PLANE: f4a = three float4 planes, void = each plane float4 or half4 by its CRYCHIC_GBUFFER_G*_F16 bit of P.flags (light_core.hpp
// gbuffer_load); whatever consumes a texel -- the quad exchange of CubeChain, the tile cull below -- consumes the widened value.
// CubeGloss: the reflection lookup takes the chain at the level of the pixel's roughness; the pixels keep the 64 x 1 footprint of a
// wavefront, and the sky reads level 0.
// Ambient (never with CubeChain): AmbientSH takes the ambient colour from the coefficient block behind the cube map.
// Specular (always with CubeGloss or CubeGlossBox): SpecularSplitSum weighs the reflection by the table behind the environment tail.
// CubeGlossBox: CubeGloss along the direction projected through the probe volume at probeVolume (twelve floats behind the tail).
// light_bind.hpp's light_variant_visit lists the combinations that exist (light_general.hip instantiates them).
template <bool ZERO_RADIUS, bool FIX, class Cube, class PLANE, class Ambient = AmbientConst, class Specular = SpecularRef>
__device__ __forceinline__ void light_frame_tile(const LightParams& P, const PLANE* __restrict__ g0, const PLANE* __restrict__ g1,
                                                 const PLANE* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                 const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                 uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0, uint32_t row1,
                                                 Ambient ambientTerm = Ambient(), Specular specTerm = Specular(),
                                                 const float* __restrict__ probeVolume = nullptr)
{
    // CubeGlossBox: the volume's scalar loads go out first and are pinned behind the issue of the depth load, whose round trip they
    // overlap (probe_pin)
    [[maybe_unused]] ProbeVolume probe{};
    if constexpr (std::is_same_v<Cube, CubeGlossBox>) probe = probe_load(probeVolume);
    const uint32_t h0 = P.flags & CRYCHIC_GBUFFER_G0_F16, h1 = P.flags & CRYCHIC_GBUFFER_G1_F16, h2 = P.flags & CRYCHIC_GBUFFER_G2_F16;
    uint32_t bx, by;
    tile_origin<0>(bx, by);
    by = light_dispatch_row(by, gridDim.y);               // the band order of dispatch_order.hpp (measured best: the natural one)
    uint32_t x, y;
    light_tile_pixel<kQuads<Cube>>(bx, by, row0, x, y);
    if (kQuads<Cube>) {
        const bool in = x < P.W && y < row1;
        const uint32_t idx = in ? y * P.W + x : 0u;
        const bool covered = in && (depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu;
        f4a G0{ 0, 0, 0, 0 }, G2{ 0, 0, 0, 0 };
        f3 r{ 0.0f, 0.0f, 0.0f };
        if (covered) { G0 = CRY_GBUFFER_TEXEL(g0, idx, h0); G2 = CRY_GBUFFER_TEXEL(g2, idx, h2); r = reflection_dir(P, G0, G2); }
        const float lod = quad_reflection_lod(P, covered, r, x, y);
        if (!in) return;
        f4 lit;
        if (covered) lit = light_pixel<ZERO_RADIUS, NoPointLights, FIX, CubeChain>(P, G0, CRY_GBUFFER_TEXEL(g1, idx, h1), G2, ambient, cube, NoPointLights(), CubeChain{ lod, cube_chain_flat(lod) });
        else if (P.flags & CRYCHIC_LIGHT_SKY) lit = sky_pixel_chain(P, cube, x, y);
        else lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
        if (radiance) radiance[idx] = f4a{ lit.x, lit.y, lit.z, lit.w };
        out[idx] = pack_rgba8(lit);
        return;
    }
    if (x >= P.W || y >= row1) return;
    const uint32_t idx = y * P.W + x;
    f4 lit;
    // coverage: the reference re-rasterises the opaque items with LESS against depth cleared to 1.0
    // (CRYCHIC.cpp:248,273) -- exactly the pixels whose normal/depth pass depth is below the clear value.
    bool coveredPixel;
    if constexpr (std::is_same_v<Cube, CubeGlossBox>) {
        const uint32_t z = depth[idx];
        probe_pin(probe);
        coveredPixel = (z & 0x00FFFFFFu) < 0x00FFFFFFu;
    } else {
        coveredPixel = (depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu;
    }
    if (coveredPixel) {
        static_assert(!Specular::kSplitSum || kGlossLookup<Cube>, "the split-sum weight goes with the gloss lookup");
        // the reference as written keeps its texel loads as argument expressions (see CRY_GBUFFER_TEXEL): naming G1 moves its code
        if constexpr (std::is_same_v<Cube, CubeLevel0> && !Ambient::kSH && !Specular::kSplitSum) {
            lit = light_pixel<ZERO_RADIUS, NoPointLights, FIX>(P, CRY_GBUFFER_TEXEL(g0, idx, h0), CRY_GBUFFER_TEXEL(g1, idx, h1), CRY_GBUFFER_TEXEL(g2, idx, h2), ambient, cube);
        } else {
            const f4a G1 = CRY_GBUFFER_TEXEL(g1, idx, h1);
            lit = light_pixel<ZERO_RADIUS, NoPointLights, FIX, Cube, Ambient, Specular>(P, CRY_GBUFFER_TEXEL(g0, idx, h0), G1, CRY_GBUFFER_TEXEL(g2, idx, h2), ambient, cube, NoPointLights(), lookup_for<Cube>(P, G1.w, 0.0f, probe), ambientTerm, specTerm);
        }
    } else if (P.flags & CRYCHIC_LIGHT_SKY) {
        lit = sky_pixel(P, cube, x, y);
    } else {
        lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };  // Colors::LightSteelBlue, CRYCHIC.cpp:247
    }
    if (radiance) radiance[idx] = f4a{ lit.x, lit.y, lit.z, lit.w };
    out[idx] = pack_rgba8(lit);
}

// ---- deferred lighting with point lights (extension, BASELINE configs[4]) ------------------------------------------
// Same pass plus NUM_POINT_LIGHTS point lights.  Tiled light culling in LDS: the 64 x 4-pixel tile of a workgroup
// reduces the world-space bounding box of its covered pixels (wave shuffles, then LDS), every lane then tests lights
// against the box (sphere of radius FalloffEnd vs AABB, conservatively inflated) and sets the light's bit in an LDS mask;
// each pixel finally walks the set bits in ascending index order -- the accumulation order of the un-culled loop -- and
// applies the exact per-pixel range test, so culling never changes a bit of the result.
// What that takes (the arithmetic is light_core.hpp's tile_box_* / tile_light_touches, which tests/hostsim runs on the host as
// well): the cull admits every light whose range test some covered pixel of the tile passes, and the range test skips only on
// `d > FalloffEnd`, which a NaN on either side does not satisfy.  So a covered position with a NaN or an infinite component makes
// its tile's box all of space (the tile admits every light; a tile whose covered positions are all NaN is not empty), a light with
// a NaN FalloffEnd or a NaN Position component is admitted by every tile that covers anything, and +-inf in a light's Position or
// FalloffEnd goes through the compares as it does per pixel.  Tiles of finite positions cull exactly as they would without these
// cases; there is one cull pass per tile and no un-culled walk.
// SPOTS (light_spots_kernel): the spot lights of their own buffer are culled by the same sphere test in the same step into a
// second mask, and walked after the point lights (the gLights order).  The cull stays spherical: a spot light contributes
// outside its cone too (the 0.001 floor of PBR.hlsl:142), so only the range test is exact.
// SHADOWED (light_spots_shadowed_kernel): spot lights k < shadows->count take their shadow factor (spot_shadow_factor), evaluated
// only where the term is (in range).  The cull is unchanged: a shadow can only scale a term it already admits.
// POINT_SHADOWED (light_point_shadows_kernel): point lights k < pointShadows->count take their cube shadow (PointShadowOf) the same
// way.  The mask word is read once per wavefront (readfirstlane: every lane reads the same LDS word), so the walk's light index is
// scalar, and with it the light's projection and map; the face is per lane (point_face's selects).
template <bool ZERO_RADIUS, class Cube, bool SPOTS, bool SHADOWED = false, bool POINT_SHADOWED = false, class PLANE = f4a,
          class Ambient = AmbientConst, class Specular = SpecularRef>
__device__ __forceinline__ void light_local_tile(const LightParams& P, const PLANE* __restrict__ g0, const PLANE* __restrict__ g1,
                                                 const PLANE* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                 const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                 uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0, uint32_t row1,
                                                 float (*s_box)[6], uint32_t* s_mask, const crychic_light* __restrict__ spots,
                                                 uint32_t numSpots, uint32_t* s_spotMask, const SpotShadows* shadows = nullptr,
                                                 const PointShadows* pointShadows = nullptr, Ambient ambientTerm = Ambient(),
                                                 Specular specTerm = Specular(), const float* __restrict__ probeVolume = nullptr)
{
    [[maybe_unused]] ProbeVolume probe{};                  // CubeGlossBox: as in light_frame_tile, ahead of the depth load and the cull
    if constexpr (std::is_same_v<Cube, CubeGlossBox>) probe = probe_load(probeVolume);
    uint32_t bx, by;
    tile_origin<0>(bx, by);
    by = light_dispatch_row(by, gridDim.y);               // the band order of dispatch_order.hpp (measured best: the natural one)
    uint32_t x, y;
    light_tile_pixel<kQuads<Cube>>(bx, by, row0, x, y);     // CubeChain: 32 x 2 pixels per wavefront (quads inside a wavefront)
    const bool inFrame = (x < P.W) && (y < row1);
    const uint32_t idx = inFrame ? y * P.W + x : 0u;
    bool covered;
    if constexpr (std::is_same_v<Cube, CubeGlossBox>) {
        const uint32_t z = depth[idx];
        probe_pin(probe);
        covered = inFrame && ((z & 0x00FFFFFFu) < 0x00FFFFFFu);
    } else {
        covered = inFrame && ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu);
    }
    const uint32_t h0 = P.flags & CRYCHIC_GBUFFER_G0_F16, h1 = P.flags & CRYCHIC_GBUFFER_G1_F16, h2 = P.flags & CRYCHIC_GBUFFER_G2_F16;
    f4a G0{ 0, 0, 0, 0 };
    if (covered) G0 = CRY_GBUFFER_TEXEL(g0, idx, h0);

    // 1. tile bounding box of the covered pixels' world positions (tile_box_pixel: all of space for a non-finite one)
    TileBox wbox = tile_box_pixel(covered, G0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        TileBox other;
#pragma unroll
        for (int c = 0; c < 3; ++c) { other.lo[c] = __shfl_xor(wbox.lo[c], off); other.hi[c] = __shfl_xor(wbox.hi[c], off); }
        wbox = tile_box_merge(wbox, other);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { for (int c = 0; c < 3; ++c) { s_box[wave][c] = wbox.lo[c]; s_box[wave][3 + c] = wbox.hi[c]; } }
    if (threadIdx.x < kMaxPointLights / 32) s_mask[threadIdx.x] = 0u;
    if (SPOTS && threadIdx.x < kMaxSpotLights / 32) s_spotMask[threadIdx.x] = 0u;
    __syncthreads();
    auto waveBox = [&](int w) { return TileBox{ { s_box[w][0], s_box[w][1], s_box[w][2] }, { s_box[w][3], s_box[w][4], s_box[w][5] } }; };
    const TileBox box = tile_box_merge(tile_box_merge(waveBox(0), waveBox(1)), tile_box_merge(waveBox(2), waveBox(3)));
    // 2. cull: light l touches the tile if dist(Position, box) <= FalloffEnd (inflated: the per-pixel test is the exact one; a NaN
    // on either side admits, as it passes the per-pixel test: tile_light_touches)
    if (tile_box_any_covered(box)) {
        for (uint32_t l = threadIdx.x; l < P.numPointLights; l += 256u) {
            const crychic_light L = P.pointLights[l];
            if (tile_light_touches(L, box)) atomicOr(&s_mask[l >> 5], 1u << (l & 31u));
        }
        if (SPOTS)
            for (uint32_t l = threadIdx.x; l < numSpots; l += 256u) {
                const crychic_light L = spots[l];
                if (tile_light_touches(L, box)) atomicOr(&s_spotMask[l >> 5], 1u << (l & 31u));
            }
    }
    __syncthreads();
    float lod = 0.0f;
    f4a G2{ 0, 0, 0, 0 };
    if (kQuads<Cube>) {                                      // every lane, converged: the quad neighbours' reflection vectors
        f3 r{ 0.0f, 0.0f, 0.0f };
        if (covered) { G2 = CRY_GBUFFER_TEXEL(g2, idx, h2); r = reflection_dir(P, G0, G2); }
        lod = quad_reflection_lod(P, covered, r, x, y);
    }
    if (!inFrame) return;

    // 3. shade
    f4 lit;
    if (covered) {
        auto culled = [&](f3 pos, f3 albedo, float roughness, float metalness, f3 normal, f3 view, f3& result, bool fixQ3, bool fixQ4) {
            const uint32_t words = (P.numPointLights + 31u) >> 5;
            for (uint32_t w = 0; w < words; ++w) {
                uint32_t m = s_mask[w];
                if (POINT_SHADOWED) m = __builtin_amdgcn_readfirstlane(m);
                while (m) {
                    const uint32_t b = (uint32_t)__builtin_ctz(m);
                    m &= m - 1u;
                    if (POINT_SHADOWED)
                        pbr_point_light(P.pointLights[w * 32u + b], pos, albedo, roughness, metalness, normal, view, result, fixQ3, fixQ4,
                                        PointShadowOf{ pointShadows, pos, &P.pointLights[w * 32u + b], w * 32u + b });
                    else
                        pbr_point_light(P.pointLights[w * 32u + b], pos, albedo, roughness, metalness, normal, view, result, fixQ3, fixQ4);
                }
            }
            if (SPOTS) {
                const uint32_t spotWords = (numSpots + 31u) >> 5;
                for (uint32_t w = 0; w < spotWords; ++w) {
                    uint32_t m = s_spotMask[w];
                    while (m) {
                        const uint32_t b = (uint32_t)__builtin_ctz(m);
                        m &= m - 1u;
                        if (SHADOWED)
                            pbr_spot_light(spots[w * 32u + b], pos, albedo, roughness, metalness, normal, view, result, fixQ3, fixQ4,
                                           SpotShadowOf{ shadows, pos, w * 32u + b });
                        else
                            pbr_spot_light(spots[w * 32u + b], pos, albedo, roughness, metalness, normal, view, result, fixQ3, fixQ4);
                    }
                }
            }
        };
        static_assert(!Specular::kSplitSum || kGlossLookup<Cube>, "the split-sum weight goes with the gloss lookup");
        const f4a G1 = CRY_GBUFFER_TEXEL(g1, idx, h1);
        if constexpr (!kQuads<Cube>) G2 = CRY_GBUFFER_TEXEL(g2, idx, h2);        // the quad exchange has loaded it already
        lit = light_pixel<ZERO_RADIUS, decltype(culled), true, Cube, Ambient, Specular>(P, G0, G1, G2, ambient, cube, culled, lookup_for<Cube>(P, G1.w, lod, probe), ambientTerm, specTerm);
    } else if (P.flags & CRYCHIC_LIGHT_SKY) {
        lit = kQuads<Cube> ? sky_pixel_chain(P, cube, x, y) : sky_pixel(P, cube, x, y);
    } else {
        lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
    }
    if (radiance) radiance[idx] = f4a{ lit.x, lit.y, lit.z, lit.w };
    out[idx] = pack_rgba8(lit);
}

#undef CRY_GBUFFER_TEXEL

}  // namespace cry
