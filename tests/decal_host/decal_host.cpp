// decal_host.cpp -- csrc/decal_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan (decal_launch) and the kernel's
// walk as decal_kernel does it: a one-dimensional grid of workgroups of four wavefronts, each an 8 x 8 pixel tile; per wavefront the
// butterfly reduction of the lanes' boxes (the xor shuffles emulated on an array of 64 boxes), lane k's test of decal k, the vote as
// a 64-bit mask, the early exit, and decal_lane for every covered lane with the mask.
#include <cstdint>
#include <cstring>
#include "decal_core.hpp"

namespace {

using namespace cry;

// One wavefront.  Returns the tile's mask.
uint64_t wavefront(const DecalArgs& a, uint32_t gx, uint32_t gy, uint32_t wave)
{
    bool covered[64];
    uint32_t idx[64];
    DecalTexel T0[64];
    TileBox box[64];
    for (uint32_t l = 0; l < 64u; ++l) {
        const uint32_t t = wave * 64u + l;
        const uint32_t px = gx * kDecalGroupW + decal_lane_x(t), py = a.row0 + gy * kDecalTile + decal_lane_y(t);
        const bool in = px < a.W && py < a.rowEnd;
        idx[l] = in ? py * a.W + px : 0u;
        uint32_t z = 0x00FFFFFFu;
        if (in) z = a.depth[idx[l]];
        covered[l] = (z & 0x00FFFFFFu) < 0x00FFFFFFu;
        T0[l] = DecalTexel{ u4{ 0u, 0u, 0u, 0u }, f4a{ 0.0f, 0.0f, 0.0f, 0.0f } };
        if (covered[l]) T0[l] = decal_load(a.g0, idx[l], a.h0);
        box[l] = tile_box_pixel(covered[l], T0[l].v);
    }
    for (int off = 32; off > 0; off >>= 1) {
        TileBox next[64];
        for (uint32_t l = 0; l < 64u; ++l) next[l] = tile_box_merge(box[l], box[l ^ (uint32_t)off]);
        std::memcpy(box, next, sizeof box);
    }
    uint64_t mask = 0;
    for (uint32_t l = 0; l < 64u; ++l)
        if (l < a.n && decal_tile_test(a.decals[l], box[l])) mask |= 1ull << l;
    if (mask == 0ull) return 0ull;
    for (uint32_t l = 0; l < 64u; ++l)
        if (covered[l]) decal_lane(a, idx[l], T0[l], mask, [](uint32_t v) { return v; });
    return mask;
}

}  // namespace

// view, proj: the pass constants' View and Proj (16 floats each).  masks: NULL, or (number of 8-row bands of the call) x (4 tilesX)
// words that take every tile's mask.  Returns the number of workgroups walked.
extern "C" uint32_t dch_apply(const float* view, const float* proj, const uint32_t* depth, void* g0, void* g1, void* g2, uint32_t formatFlags,
                              const crychic_decal* decals, uint32_t nDecals, const crychic_texture* textures, uint32_t nTextures, uint32_t W,
                              uint32_t H, uint32_t row0, uint32_t rows, uint64_t* masks)
{
    const DecalLaunch L = decal_launch(view, proj, depth, g0, g1, g2, formatFlags, decals, nDecals, textures, nTextures, W, H, row0, rows);
    const DecalArgs& a = L.args;
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t gy = g / a.tilesX, gx = g - gy * a.tilesX;
        for (uint32_t wave = 0; wave < kDecalWaves; ++wave) {
            const uint64_t m = wavefront(a, gx, gy, wave);
            if (masks) masks[(size_t)gy * (a.tilesX * kDecalWaves) + gx * kDecalWaves + wave] = m;
        }
    }
    return L.groups;
}
