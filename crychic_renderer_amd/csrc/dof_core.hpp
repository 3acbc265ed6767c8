// dof_core.hpp -- the body of crychic_dof (include/crychic_hip.h states the definition), built for the device
// (dof.hip) and for the host (tests/dof_host): one call per thread and phase, the caller supplies the barrier between the phases and
// the reduction of the window's largest circle of confusion.
//
// Structure: one workgroup of 256 threads per 64 x 16 output tile.  Phase 1 (dof_stage) loads the tile with an apron of R texels on
// every side into LDS, 16 bytes per texel: { the RGBA8 texel, D24, P, unused } with P = ((128 - c) << 16) | inv[c] and c the texel's
// circle of confusion, computed here once per staged texel and not once per tap.  P falls as c rises and inv[] never rises with c, so
// the definition's "c_e = behind ? min(c_s, c_p) : c_s" AND its table look-up inv[c_e] are one select and one max on P: the tap loop
// reads nothing but the texel.  A window position outside the frame holds c = 0 and colour 0 (dof_outside_texel): it is never a centre,
// every other offset has d16 >= 16, and c_e <= c_s = 0 whichever way the depth compare goes, so k = clamp(0 + 8 - d16, 0, 16) = 0 and
// w = 0 -- it adds 0 to every sum, which is what skipping it adds; the loop needs no coordinates.
// Phase 2 (dof_gather): a lane owns column t % 64 of four consecutive rows 4 (t / 64) .. + 3.  The taps run over kDofTaps, every
// offset of the radius-8 disc sorted by its squared length, so the disc of any R is a prefix and d16 never falls along the table;
// the entry is wave-uniform (a scalar load), the lanes of a wavefront read consecutive 16-byte texels, and a lane's four pixels are
// four reads at constant distances from one address.  The loop ends at the first entry with d16 >= cmax + 8, cmax the largest c of
// the staged window: c_e <= c_s <= cmax, so every later tap has k = 0.  cmax <= 8 leaves the centre tap alone, whose quotient is the
// texel itself (w ch + (w >> 1)) / w = ch: the tile is copied without a division.  Both are exact because the sums are integers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"

namespace cry {

// The output tile of a workgroup is a build parameter so that shapes can be measured against each other:
// 64 x 16, the default, or 32 x 32.  A lane owns column t % W of the four consecutive rows 4 (t / W) .. + 3.
#if !defined(CRY_DOF_TILE_W)
#define CRY_DOF_TILE_W 64
#define CRY_DOF_TILE_H 16
#endif

constexpr uint32_t kDofMaxRadius = 8u;              // CRYCHIC_DOF_MAX_RADIUS (api.cpp asserts the two agree)
constexpr uint32_t kDofTileW = CRY_DOF_TILE_W, kDofTileH = CRY_DOF_TILE_H;
constexpr uint32_t kDofThreads = 256u, kDofWaves = kDofThreads / 64u;
constexpr uint32_t kDofRowsPerLane = kDofTileW * kDofTileH / kDofThreads;       // 4
static_assert(kDofTileW * kDofTileH == 4u * kDofThreads && (kDofTileW == 64u || kDofTileW == 32u), "four pixels per lane, 64 or 32 columns");
constexpr uint32_t kDofLdsW = kDofTileW + 2u * kDofMaxRadius;                   // 80: the row pitch whatever R is
constexpr uint32_t kDofLdsH = kDofTileH + 2u * kDofMaxRadius;                   // 32
constexpr uint32_t kDofLdsTexels = kDofLdsW * kDofLdsH;                         // 16 bytes each: 40 KiB
constexpr uint32_t kDofMaxTaps = 197u;

struct DofParams { float focusDistance, aperture; uint32_t maxRadius, reserved[5]; };      // crychic_dof_params

typedef uint32_t DofTexel __attribute__((ext_vector_type(4)));

// Every offset of the radius-8 disc, sorted by ox^2 + oy^2 (rows first within one length): (d16 << 16) | ((oy + 8) << 8) | (ox + 8)
// with d16 = isqrt(256 (ox^2 + oy^2)).  count[R] offsets lie inside radius R.
struct DofTaps { uint32_t e[kDofMaxTaps + 1u]; uint32_t count[kDofMaxRadius + 1u]; };      // e[197]: a sentinel no cut reaches past
constexpr uint32_t dof_isqrt(uint32_t v)
{
    uint32_t r = 0u;
    while ((r + 1u) * (r + 1u) <= v) ++r;
    return r;
}
constexpr DofTaps dof_make_taps()
{
    DofTaps t = {};
    uint32_t n = 0u;
    const int32_t R = (int32_t)kDofMaxRadius;
    for (int32_t r2 = 0; r2 <= R * R; ++r2) {
        for (int32_t oy = -R; oy <= R; ++oy)
            for (int32_t ox = -R; ox <= R; ++ox)
                if (ox * ox + oy * oy == r2) t.e[n++] = (dof_isqrt(256u * (uint32_t)r2) << 16) | ((uint32_t)(oy + R) << 8) | (uint32_t)(ox + R);
        const uint32_t r = dof_isqrt((uint32_t)r2);
        if (r * r == (uint32_t)r2) t.count[r] = n;          // the table is sorted: everything up to here lies inside radius r
    }
    t.e[n] = 0xFFFF0000u;
    return t;
}
static constexpr DofTaps kDofTaps = dof_make_taps();
static_assert(kDofTaps.count[1] == 5u && kDofTaps.count[2] == 13u && kDofTaps.count[3] == 29u && kDofTaps.count[4] == 49u && kDofTaps.count[5] == 81u &&
              kDofTaps.count[6] == 113u && kDofTaps.count[7] == 149u && kDofTaps.count[8] == kDofMaxTaps, "the discs of the definition");
static_assert(kDofTaps.e[0] == ((8u << 8) | 8u) && (kDofTaps.e[kDofMaxTaps - 1u] >> 16) == 128u, "the centre first, the longest offset last");

// the kernel's arguments (kernarg segment: every field is wave-uniform)
struct DofArgs {
    const uint32_t* depth;
    const uint32_t* in;
    uint32_t* out;
    uint32_t W, H, row0, rowEnd, yEnd, tilesX, R, nTaps;       // yEnd: one past the last row the call may read
    float A, g, ap16, hi;
};

struct DofLaunch { DofArgs args; uint32_t groups; };           // groups == 0: nothing to launch

// The launcher's plan and the host-side constants of the definition.  proj: the pass constants' Proj.  The caller has checked every
// argument (api.cpp).
inline DofLaunch dof_launch(const float* proj, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                            uint32_t rows, const DofParams& p)
{
    DofLaunch L;
    DofArgs& a = L.args;
    a.depth = depth;
    a.in = reinterpret_cast<const uint32_t*>(in);
    a.out = reinterpret_cast<uint32_t*>(out);
    a.W = W; a.H = H; a.row0 = row0; a.rowEnd = row0 + rows;
    a.R = p.maxRadius;
    a.yEnd = a.rowEnd + a.R < H ? a.rowEnd + a.R : H;
    a.nTaps = kDofTaps.count[a.R];
    a.tilesX = (W + kDofTileW - 1u) / kDofTileW;
    a.A = proj[10];
    a.g = p.focusDistance / proj[11];
    a.ap16 = p.aperture * 16.0f;
    a.hi = (float)(16u * a.R);
    L.groups = a.tilesX * ((rows + kDofTileH - 1u) / kDofTileH);
    return L;
}

// The circle of confusion of a depth texel, 0 .. 16 R, in 1/16 pixel.
CRY_HD uint32_t dof_coc(const DofArgs& a, uint32_t depthWord)
{
    const float d = d24_to_float(depthWord);
    const float x = (d - a.A) * a.g;
    const float e = __builtin_fabsf(1.0f - x);
    const float u = e * a.ap16;
    return (uint32_t)(clampf(u, 0.0f, a.hi) + 0.5f);
}

CRY_HD uint32_t dof_pack(uint32_t c)
{
    const uint32_t m = c > 16u ? c : 16u;
    return ((128u - c) << 16) | ((1u << 20) / (m * m));
}
CRY_HD DofTexel dof_outside_texel() { return DofTexel{ 0u, 0u, (128u << 16) | 4096u, 0u }; }

// Phase 1, thread t of 256 of tile (tileX, tileY): its share of the window, rows tileY0 - R .. tileY0 + 15 + R and columns
// tileX0 - R .. tileX0 + 63 + R, into `win` (window row r, column 8 - R + i at r * 80 + 8 - R + i).  Returns the largest c it staged.
CRY_HD uint32_t dof_stage(const DofArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, DofTexel* win)
{
    const int32_t x0 = (int32_t)(tileX * kDofTileW) - (int32_t)kDofMaxRadius;
    const int32_t y0 = (int32_t)(a.row0 + tileY * kDofTileH) - (int32_t)a.R;
    const uint32_t texels = kDofLdsW * (kDofTileH + 2u * a.R);
    const uint32_t colLo = kDofMaxRadius - a.R, colHi = kDofMaxRadius + kDofTileW + a.R;
    uint32_t cmax = 0u;
    for (uint32_t i = t; i < texels; i += kDofThreads) {
        const uint32_t wy = i / kDofLdsW, wx = i - wy * kDofLdsW;
        if (wx < colLo || wx >= colHi) continue;            // no tap of radius R reaches it
        const int32_t sx = x0 + (int32_t)wx, sy = y0 + (int32_t)wy;
        DofTexel v = dof_outside_texel();
        if (sx >= 0 && sx < (int32_t)a.W && sy >= 0 && sy < (int32_t)a.yEnd) {
            const uint32_t at = (uint32_t)sy * a.W + (uint32_t)sx;
            const uint32_t dw = a.depth[at];
            const uint32_t c = dof_coc(a, dw);
            v = DofTexel{ a.in[at], dw & 0x00FFFFFFu, dof_pack(c), 0u };
            cmax = c > cmax ? c : cmax;
        }
        win[i] = v;
    }
    return cmax;
}

// Phase 2, thread t: its four pixels from the staged window (complete: the caller's barrier); cmax: the largest c of the window, or
// anything above it.
CRY_HD void dof_gather(const DofArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, const DofTexel* win, uint32_t cmax)
{
    const uint32_t lx = t % kDofTileW, ly = kDofRowsPerLane * (t / kDofTileW);
    const uint32_t px = tileX * kDofTileW + lx, py = a.row0 + tileY * kDofTileH + ly;
    if (py >= a.rowEnd) return;                             // the whole wavefront where the tile is 64 wide
    const uint32_t centre = (a.R + ly) * kDofLdsW + kDofMaxRadius + lx;
    const uint32_t cut = cmax + 8u;
    uint32_t result[kDofRowsPerLane];
    if (cut <= 16u) {
        for (uint32_t j = 0; j < kDofRowsPerLane; ++j) result[j] = win[centre + j * kDofLdsW][0];
    } else {
        uint32_t Dp[kDofRowsPerLane], Pp[kDofRowsPerLane], sw[kDofRowsPerLane], sr[kDofRowsPerLane], sg[kDofRowsPerLane], sb[kDofRowsPerLane];
        for (uint32_t j = 0; j < kDofRowsPerLane; ++j) {
            const DofTexel c = win[centre + j * kDofLdsW];
            Dp[j] = c[1]; Pp[j] = c[2];
            sw[j] = sr[j] = sg[j] = sb[j] = 0u;
        }
        uint32_t next = kDofTaps.e[0];
        for (uint32_t i = 0; i < a.nTaps; ++i) {
            const uint32_t e = next, d16 = e >> 16;
            if (d16 >= cut) break;
            next = kDofTaps.e[i + 1u];                      // the scalar load of the next entry runs under this one's taps
            const int32_t ox = (int32_t)(e & 255u) - (int32_t)kDofMaxRadius, oy = (int32_t)((e >> 8) & 255u) - (int32_t)kDofMaxRadius;
            const DofTexel* tap = win + ((int32_t)centre + oy * (int32_t)kDofLdsW + ox);
            const uint32_t kb = 136u - d16;                 // k = c_e + 8 - d16 with c_e = 128 - (P >> 16); d16 <= 128
            for (uint32_t j = 0; j < kDofRowsPerLane; ++j) {
                const DofTexel s = tap[j * kDofLdsW];
                const uint32_t own = s[1] > Dp[j] ? Pp[j] : 0u;
                const uint32_t P = s[2] > own ? s[2] : own;
                // k in unsigned arithmetic (kb >= 8): a saturating subtraction and a minimum, whose range the compiler carries into the
                // products -- behind a signed clamp it takes w for a 32-bit number and w ch through the quarter-rate 64-bit multiply-add
                const uint32_t cq = P >> 16;
                uint32_t k = kb > cq ? kb - cq : 0u;
                k = k < 16u ? k : 16u;
                const uint32_t w = mul24(k, P & 0xFFFFu);
                sw[j] += w;
                sr[j] += mul24(w, s[0] & 255u);
                sg[j] += mul24(w, (s[0] >> 8) & 255u);
                sb[j] += mul24(w, (s[0] >> 16) & 255u);
            }
        }
        for (uint32_t j = 0; j < kDofRowsPerLane; ++j) {
            const uint32_t half = sw[j] >> 1;
            const uint32_t r = (sr[j] + half) / sw[j], g = (sg[j] + half) / sw[j], b = (sb[j] + half) / sw[j];
            result[j] = r | (g << 8) | (b << 16) | (win[centre + j * kDofLdsW][0] & 0xFF000000u);
        }
    }
    if (px >= a.W) return;
    for (uint32_t j = 0; j < kDofRowsPerLane; ++j)
        if (py + j < a.rowEnd) a.out[(size_t)(py + j) * a.W + px] = result[j];
}

}  // namespace cry
