// ssr_pyramid_core.hpp -- the body of crychic_ssr_pyramid's kernel (include/crychic_hip.h states the definition; DESIGN.md section
// 31), built for the device (ssr_pyramid.hip) and for the host (tests/ssr_gloss_host): one call per thread and phase, the caller
// supplies the barriers between the phases.
//
// One workgroup of 256 threads per 32 x 16 destination tile (the bloom's downsample shape, with RGBA8 texels):
//   stage    the 66 x 34 source window, every coordinate clamped to the source level, one dword per texel -- a 16-byte load of four
//            texels per lane where the level's address and row pitch allow it, the two apron columns one texel each;
//   rows     (1, 3, 3, 1) along x into 34 x 32 sums of two dwords: R and B in the halves of one (mask 0x00FF00FF), G and A in those
//            of the other, at most 8 * 255 a half;
//   columns  (1, 3, 3, 1) along y, at most 64 * 255 a half, rounded, packed back into a texel and stored, two texels per thread.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kSsrGlossMaxLevels = 8u;         // CRYCHIC_SSR_GLOSS_MAX_LEVELS (api.cpp asserts the two agree)
constexpr uint32_t kSsrPyrThreads = 256u;
constexpr uint32_t kSsrPyrTileW = 32u, kSsrPyrTileH = 16u;                              // the destination tile of a workgroup
constexpr uint32_t kSsrPyrWinW = 2u * kSsrPyrTileW + 2u, kSsrPyrWinH = 2u * kSsrPyrTileH + 2u;      // 66 x 34 source texels
constexpr uint32_t kSsrPyrWinTexels = kSsrPyrWinW * kSsrPyrWinH;                        // 4 bytes each: 8 976 bytes
constexpr uint32_t kSsrPyrRowSums = kSsrPyrWinH * kSsrPyrTileW;                         // 8 bytes each: 8 704 bytes
constexpr uint32_t kSsrPyrQuadsPerRow = 2u * kSsrPyrTileW / 4u;                         // 16 aligned groups of four texels per window row
constexpr uint32_t kSsrPyrMask = 0x00FF00FFu;
static_assert(kSsrPyrTileW * kSsrPyrTileH == 2u * kSsrPyrThreads, "two destination texels per thread");

typedef uint32_t SsrPyrQuad __attribute__((ext_vector_type(4)));        // four RGBA8 texels
typedef uint32_t SsrPyrSum __attribute__((ext_vector_type(2)));         // { R | B << 16, G | A << 16 }

// Level sizes and workspace offsets in bytes; level 0 is the frame (offset unused).  valid == 0: W, H or levels outside their ranges.
struct SsrPyramidPlan { uint32_t valid, nEff; uint32_t w[kSsrGlossMaxLevels], h[kSsrGlossMaxLevels]; size_t off[kSsrGlossMaxLevels]; size_t bytes; };
inline SsrPyramidPlan ssr_pyramid_plan(uint32_t W, uint32_t H, uint32_t levels)
{
    SsrPyramidPlan p = {};
    if (W == 0u || H == 0u || levels == 0u || levels > kSsrGlossMaxLevels) return p;
    p.valid = 1u;
    p.w[0] = W; p.h[0] = H;
    size_t at = 0;
    uint32_t k = 0u;
    while (k + 1u < levels && !(p.w[k] == 1u && p.h[k] == 1u)) {
        ++k;
        p.w[k] = (p.w[k - 1u] + 1u) >> 1;
        p.h[k] = (p.h[k - 1u] + 1u) >> 1;
        p.off[k] = at;
        p.bytes = at + (size_t)p.w[k] * p.h[k] * 4u;
        at = (p.bytes + 15u) & ~(size_t)15u;
    }
    p.nEff = k;
    return p;
}

struct SsrPyrArgs {
    const uint32_t* src;            // level k: the frame or a level of the workspace
    uint32_t* dst;                  // level k + 1
    uint32_t sw, sh, dw, dh, tilesX;
    uint32_t vec;                   // src is 16-byte aligned and sw a multiple of 4
};
struct SsrPyrLaunch { SsrPyrArgs args; uint32_t groups; };

inline SsrPyrLaunch ssr_pyr_launch(const void* src, void* dst, uint32_t sw, uint32_t sh)
{
    SsrPyrLaunch L;
    SsrPyrArgs& a = L.args;
    a.src = static_cast<const uint32_t*>(src);
    a.dst = static_cast<uint32_t*>(dst);
    a.sw = sw; a.sh = sh; a.dw = (sw + 1u) >> 1; a.dh = (sh + 1u) >> 1;
    a.tilesX = (a.dw + kSsrPyrTileW - 1u) / kSsrPyrTileW;
    a.vec = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u && (sw & 3u) == 0u) ? 1u : 0u;
    L.groups = a.tilesX * ((a.dh + kSsrPyrTileH - 1u) / kSsrPyrTileH);        // at most 2^28 / 4 / 512 + a row and a column of tiles
    return L;
}

CRY_HD uint32_t ssr_pyr_clamp(int32_t v, uint32_t n) { return v < 0 ? 0u : ((uint32_t)v < n ? (uint32_t)v : n - 1u); }

// Phase 1, thread t of tile (tileX, tileY): its share of the window -- window (wx, wy) is source (clamp(2 x0 - 1 + wx),
// clamp(2 y0 - 1 + wy)) -- into win[wy * 66 + wx].  Every index into src is a clamped coordinate pair: below sw * sh.
CRY_HD void ssr_pyr_stage(const SsrPyrArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, uint32_t* win)
{
    const int32_t sx0 = (int32_t)(2u * tileX * kSsrPyrTileW) - 1, sy0 = (int32_t)(2u * tileY * kSsrPyrTileH) - 1;
    constexpr uint32_t perRow = kSsrPyrQuadsPerRow + 2u;        // 16 groups of four and the two apron columns
    for (uint32_t i = t; i < perRow * kSsrPyrWinH; i += kSsrPyrThreads) {
        const uint32_t wy = i / perRow, j = i - wy * perRow;
        const size_t row = (size_t)ssr_pyr_clamp(sy0 + (int32_t)wy, a.sh) * a.sw;
        uint32_t* to = win + wy * kSsrPyrWinW;
        if (j < kSsrPyrQuadsPerRow) {
            const uint32_t wx = 1u + 4u * j, sx = (uint32_t)(sx0 + (int32_t)wx);        // sx is a multiple of 4
            SsrPyrQuad q;
            if (a.vec && sx + 3u < a.sw) {
                q = *reinterpret_cast<const SsrPyrQuad*>(a.src + row + sx);
            } else {
                for (uint32_t c = 0; c < 4u; ++c) q[c] = a.src[row + ssr_pyr_clamp((int32_t)(sx + c), a.sw)];
            }
            for (uint32_t c = 0; c < 4u; ++c) to[wx + c] = q[c];
        } else {
            const uint32_t wx = j == kSsrPyrQuadsPerRow ? 0u : kSsrPyrWinW - 1u;
            to[wx] = a.src[row + ssr_pyr_clamp(sx0 + (int32_t)wx, a.sw)];
        }
    }
}

// Phase 2, thread t: the rows of the staged window filtered (1, 3, 3, 1) to the tile's 32 columns: sums[wy * 32 + ox].
CRY_HD void ssr_pyr_rows(uint32_t t, const uint32_t* win, SsrPyrSum* sums)
{
    for (uint32_t i = t; i < kSsrPyrRowSums; i += kSsrPyrThreads) {
        const uint32_t wy = i / kSsrPyrTileW, ox = i - wy * kSsrPyrTileW;
        const uint32_t* s = win + wy * kSsrPyrWinW + 2u * ox;
        const uint32_t p0 = s[0], p1 = s[1], p2 = s[2], p3 = s[3];
        const uint32_t rb = (p0 & kSsrPyrMask) + 3u * ((p1 & kSsrPyrMask) + (p2 & kSsrPyrMask)) + (p3 & kSsrPyrMask);
        const uint32_t ga = ((p0 >> 8) & kSsrPyrMask) + 3u * (((p1 >> 8) & kSsrPyrMask) + ((p2 >> 8) & kSsrPyrMask)) + ((p3 >> 8) & kSsrPyrMask);
        sums[i] = SsrPyrSum{ rb, ga };
    }
}

// Phase 3, thread t: two texels of the tile from the row sums (complete: the caller's barrier), rounded and stored.  A half holds at
// most 64 * 255 + 32 before the shift; the shift moves the upper half's low bits into bits 10 .. 15 of the lower, which the mask drops.
CRY_HD void ssr_pyr_columns(const SsrPyrArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, const SsrPyrSum* sums)
{
    for (uint32_t i = t; i < kSsrPyrTileW * kSsrPyrTileH; i += kSsrPyrThreads) {
        const uint32_t oy = i / kSsrPyrTileW, ox = i - oy * kSsrPyrTileW;
        const uint32_t dx = tileX * kSsrPyrTileW + ox, dy = tileY * kSsrPyrTileH + oy;
        if (dx >= a.dw || dy >= a.dh) continue;
        const SsrPyrSum* s = sums + 2u * oy * kSsrPyrTileW + ox;
        const SsrPyrSum s0 = s[0], s1 = s[kSsrPyrTileW], s2 = s[2u * kSsrPyrTileW], s3 = s[3u * kSsrPyrTileW];
        const uint32_t rb = ((s0[0] + 3u * (s1[0] + s2[0]) + s3[0] + 0x00200020u) >> 6) & kSsrPyrMask;
        const uint32_t ga = ((s0[1] + 3u * (s1[1] + s2[1]) + s3[1] + 0x00200020u) >> 6) & kSsrPyrMask;
        a.dst[(size_t)dy * a.dw + dx] = rb | (ga << 8);
    }
}

}  // namespace cry
