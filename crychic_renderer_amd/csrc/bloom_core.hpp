// bloom_core.hpp -- the bodies of crychic_bloom's kernels (include/crychic_hip.h states the definition), built
// for the device (bloom.hip) and for the host (tests/bloom_host): one call per thread and phase, the caller supplies the barriers
// between the phases and the votes.
//
// Four roles, three bodies:
//   downsample (bloom_down_*): one workgroup of 256 threads per 32 x 16 destination tile.  Phase 1 stages the 66 x 34 source window
//   in LDS, every coordinate clamped to the source level, 8 bytes per texel in the pyramid's own layout (R | G << 16, B).  The first
//   level (First = true) reads the RGBA8 frame and weighs every texel as it arrives -- a 16-byte load of four texels per lane where
//   the plane and the row pitch allow it, the two apron columns one texel each -- the later levels copy pyramid texels.  Every thread
//   reports whether it staged anything but zeros; the caller ORs that over the workgroup (a wave vote and four LDS words), and a tile
//   of zeros is stored without the two filter phases: the workspace is not assumed to be cleared.  Phase 2 filters the rows
//   (1, 3, 3, 1) into 34 x 32 sums of three dwords, phase 3 filters the columns, rounds and stores two texels per thread.
//   unwind (bloom_unwind): one thread per texel of level k, in place: it reads its own D_k and four texels of U_(k+1).
//   composite (bloom_composite_*): one thread per four consecutive pixels of the plane taken as one line of W H pixels, 16 bytes per
//   lane where both planes are 16-byte aligned (pixels outside the row range of the call are masked), else one pixel per thread.
//   Four pixels of one row share the eight texels of U_1 around them.  A wavefront that adds nothing anywhere stores nothing when
//   the call is in place (the caller's vote); out of place it stores what it loaded.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kBloomMaxLevels = 8u;            // CRYCHIC_BLOOM_MAX_LEVELS (api.cpp asserts the two agree)
constexpr uint32_t kBloomThreads = 256u, kBloomWaves = kBloomThreads / 64u;
constexpr uint32_t kBloomTileW = 32u, kBloomTileH = 16u;                        // the destination tile of a downsample workgroup
constexpr uint32_t kBloomWinW = 2u * kBloomTileW + 2u, kBloomWinH = 2u * kBloomTileH + 2u;      // 66 x 34 source texels
constexpr uint32_t kBloomWinTexels = kBloomWinW * kBloomWinH;                   // 8 bytes each: 17 952 bytes
constexpr uint32_t kBloomRowSums = kBloomWinH * kBloomTileW * 3u;               // dwords: 13 056 bytes
constexpr uint32_t kBloomQuadsPerRow = 2u * kBloomTileW / 4u;                   // 16 aligned groups of four frame texels per window row
static_assert(kBloomTileW * kBloomTileH == 2u * kBloomThreads, "two destination texels per thread");

struct BloomParams { uint32_t threshold, knee, scatter, intensity, levels, reserved[3]; };      // crychic_bloom_params

typedef uint32_t BloomTexel __attribute__((ext_vector_type(2)));               // { R | G << 16, B }: four uint16_t, the last one 0
typedef uint32_t BloomQuad __attribute__((ext_vector_type(4)));                // four RGBA8 pixels

// Level sizes and workspace offsets; level 0 is the frame (offset unused).  nEff == 0: W, H or levels outside their ranges.
struct BloomPlan { uint32_t nEff; uint32_t w[kBloomMaxLevels + 1u], h[kBloomMaxLevels + 1u]; size_t off[kBloomMaxLevels + 1u]; size_t bytes; };
inline BloomPlan bloom_plan(uint32_t W, uint32_t H, uint32_t levels)
{
    BloomPlan p = {};
    if (W == 0u || H == 0u || levels == 0u || levels > kBloomMaxLevels) return p;
    const uint32_t m = W > H ? W : H;
    uint32_t lg = 0u;
    while (lg < 32u && (1ull << lg) < m) ++lg;              // ceil(log2(m))
    if (lg == 0u) lg = 1u;
    p.nEff = levels < lg ? levels : lg;
    p.w[0] = W; p.h[0] = H;
    size_t at = 0;
    for (uint32_t k = 1; k <= p.nEff; ++k) {
        p.w[k] = (p.w[k - 1u] + 1u) >> 1;
        p.h[k] = (p.h[k - 1u] + 1u) >> 1;
        p.off[k] = at;
        at += ((size_t)p.w[k] * p.h[k] * 8u + 15u) & ~(size_t)15u;
    }
    p.bytes = p.off[p.nEff] + (size_t)p.w[p.nEff] * p.h[p.nEff] * 8u;
    return p;
}

CRY_HD uint32_t bloom_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// (L - 256 T) / K without a division per texel: kmagic = 2^24 / K + 1 (floor), and n = L - 256 T <= 65280 < 2^16.  With
// e = kmagic K - 2^24 in 1 .. K, n kmagic / 2^24 = n / K + n e / (2^24 K), and n e / (2^24 K) <= n / 2^24 < 1 / K (n K <= 65280 * 255
// < 2^24): the floor is that of n / K.  (n << 8) kmagic >> 32 is that quotient in one multiply-high; tests/test_bloom_host.py runs
// every n and K against the division.
CRY_HD uint32_t bloom_weight(uint32_t L, uint32_t t256, uint32_t kmagic)
{
    if (L <= t256) return 0u;
    const uint32_t q = bloom_mulhi((L - t256) << 8, kmagic);
    return q < 256u ? q : 256u;
}

CRY_HD BloomTexel bloom_bright(uint32_t px, uint32_t t256, uint32_t kmagic)
{
    const uint32_t R = px & 255u, G = (px >> 8) & 255u, B = (px >> 16) & 255u;
    const uint32_t w = bloom_weight(mul24(77u, R) + mul24(150u, G) + mul24(29u, B), t256, kmagic);
    return BloomTexel{ mul24(R, w) | (mul24(G, w) << 16), mul24(B, w) };
}

// ---- downsample -----------------------------------------------------------------------------------------------------------------
struct BloomDownArgs {
    const void* src;                // the RGBA8 frame (First) or level k
    BloomTexel* dst;                // level k + 1
    uint32_t sw, sh, dw, dh, tilesX;
    uint32_t t256, kmagic;          // First only
    uint32_t vec;                   // First only: src is 16-byte aligned and sw a multiple of 4
};
struct BloomDownLaunch { BloomDownArgs args; uint32_t groups; };

inline BloomDownLaunch bloom_down_launch(const void* src, void* dst, uint32_t sw, uint32_t sh, const BloomParams* first)
{
    BloomDownLaunch L;
    BloomDownArgs& a = L.args;
    a.src = src;
    a.dst = static_cast<BloomTexel*>(dst);
    a.sw = sw; a.sh = sh; a.dw = (sw + 1u) >> 1; a.dh = (sh + 1u) >> 1;
    a.tilesX = (a.dw + kBloomTileW - 1u) / kBloomTileW;
    a.t256 = first ? 256u * first->threshold : 0u;
    a.kmagic = first ? (1u << 24) / first->knee + 1u : 0u;
    a.vec = (first && (reinterpret_cast<uintptr_t>(src) & 15u) == 0u && (sw & 3u) == 0u) ? 1u : 0u;
    L.groups = a.tilesX * ((a.dh + kBloomTileH - 1u) / kBloomTileH);
    return L;
}

CRY_HD uint32_t bloom_clamp_coord(int32_t v, uint32_t n) { return v < 0 ? 0u : ((uint32_t)v < n ? (uint32_t)v : n - 1u); }

// Phase 1, thread t of tile (tileX, tileY): its share of the window -- window (wx, wy) is source (clamp(2 x0 - 1 + wx),
// clamp(2 y0 - 1 + wy)) -- into win[wy * 66 + wx].  Returns non-zero if it staged a texel that is not zero.
template <bool First>
CRY_HD uint32_t bloom_down_stage(const BloomDownArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, BloomTexel* win)
{
    const int32_t sx0 = (int32_t)(2u * tileX * kBloomTileW) - 1, sy0 = (int32_t)(2u * tileY * kBloomTileH) - 1;
    uint32_t any = 0u;
    if (First) {
        const uint32_t* src = static_cast<const uint32_t*>(a.src);
        constexpr uint32_t perRow = kBloomQuadsPerRow + 2u;     // 16 groups of four and the two apron columns
        for (uint32_t i = t; i < perRow * kBloomWinH; i += kBloomThreads) {
            const uint32_t wy = i / perRow, j = i - wy * perRow;
            const uint32_t row = bloom_clamp_coord(sy0 + (int32_t)wy, a.sh) * a.sw;
            BloomTexel* to = win + wy * kBloomWinW;
            if (j < kBloomQuadsPerRow) {
                const uint32_t wx = 1u + 4u * j, sx = (uint32_t)(sx0 + (int32_t)wx);        // sx is a multiple of 4
                BloomQuad q;
                if (a.vec && sx + 3u < a.sw) {
                    q = *reinterpret_cast<const BloomQuad*>(src + row + sx);
                } else {
                    for (uint32_t c = 0; c < 4u; ++c) q[c] = src[row + bloom_clamp_coord((int32_t)(sx + c), a.sw)];
                }
                for (uint32_t c = 0; c < 4u; ++c) {
                    const BloomTexel b = bloom_bright(q[c], a.t256, a.kmagic);
                    to[wx + c] = b;
                    any |= b[0] | b[1];
                }
            } else {
                const uint32_t wx = j == kBloomQuadsPerRow ? 0u : kBloomWinW - 1u;
                const BloomTexel b = bloom_bright(src[row + bloom_clamp_coord(sx0 + (int32_t)wx, a.sw)], a.t256, a.kmagic);
                to[wx] = b;
                any |= b[0] | b[1];
            }
        }
    } else {
        const BloomTexel* src = static_cast<const BloomTexel*>(a.src);
        for (uint32_t i = t; i < kBloomWinTexels; i += kBloomThreads) {
            const uint32_t wy = i / kBloomWinW, wx = i - wy * kBloomWinW;
            const BloomTexel b = src[bloom_clamp_coord(sy0 + (int32_t)wy, a.sh) * a.sw + bloom_clamp_coord(sx0 + (int32_t)wx, a.sw)];
            win[i] = b;
            any |= b[0] | b[1];
        }
    }
    return any;
}

// Phase 2, thread t: the rows of the staged window filtered (1, 3, 3, 1) to the tile's 32 columns: sums[(wy * 32 + ox) * 3 + ch], at
// most 8 * 65280.
CRY_HD void bloom_down_rows(uint32_t t, const BloomTexel* win, uint32_t* sums)
{
    for (uint32_t i = t; i < kBloomWinH * kBloomTileW; i += kBloomThreads) {
        const uint32_t wy = i / kBloomTileW, ox = i - wy * kBloomTileW;
        const BloomTexel* s = win + wy * kBloomWinW + 2u * ox;
        const BloomTexel p0 = s[0], p1 = s[1], p2 = s[2], p3 = s[3];
        sums[3u * i + 0u] = (p0[0] & 0xFFFFu) + 3u * ((p1[0] & 0xFFFFu) + (p2[0] & 0xFFFFu)) + (p3[0] & 0xFFFFu);
        sums[3u * i + 1u] = (p0[0] >> 16) + 3u * ((p1[0] >> 16) + (p2[0] >> 16)) + (p3[0] >> 16);
        sums[3u * i + 2u] = p0[1] + 3u * (p1[1] + p2[1]) + p3[1];
    }
}

// Phase 3, thread t: two texels of the tile from the row sums (complete: the caller's barrier), rounded and stored.
CRY_HD void bloom_down_columns(const BloomDownArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, const uint32_t* sums)
{
    for (uint32_t i = t; i < kBloomTileW * kBloomTileH; i += kBloomThreads) {
        const uint32_t oy = i / kBloomTileW, ox = i - oy * kBloomTileW;
        const uint32_t dx = tileX * kBloomTileW + ox, dy = tileY * kBloomTileH + oy;
        if (dx >= a.dw || dy >= a.dh) continue;
        const uint32_t* s = sums + (2u * oy * kBloomTileW + ox) * 3u;
        constexpr uint32_t pitch = 3u * kBloomTileW;
        uint32_t v[3];
        for (uint32_t ch = 0; ch < 3u; ++ch)
            v[ch] = (s[ch] + 3u * (s[pitch + ch] + s[2u * pitch + ch]) + s[3u * pitch + ch] + 32u) >> 6;
        a.dst[(size_t)dy * a.dw + dx] = BloomTexel{ v[0] | (v[1] << 16), v[2] };
    }
}

// A tile whose window is all zeros: the same stores as phase 3, of zeros.
CRY_HD void bloom_down_zero(const BloomDownArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t)
{
    for (uint32_t i = t; i < kBloomTileW * kBloomTileH; i += kBloomThreads) {
        const uint32_t oy = i / kBloomTileW, ox = i - oy * kBloomTileW;
        const uint32_t dx = tileX * kBloomTileW + ox, dy = tileY * kBloomTileH + oy;
        if (dx < a.dw && dy < a.dh) a.dst[(size_t)dy * a.dw + dx] = BloomTexel{ 0u, 0u };
    }
}

// ---- 2x upsample ----------------------------------------------------------------------------------------------------------------
// The neighbour of x' = x >> 1: x' + 1 for an odd x, x' - 1 for an even one, clamped to [0, n - 1].
CRY_HD uint32_t bloom_neighbour(uint32_t x, uint32_t n)
{
    const uint32_t h = x >> 1;
    if (x & 1u) return h + 1u < n ? h + 1u : n - 1u;
    return h ? h - 1u : 0u;
}

struct BloomRgb { uint32_t r, g, b; };
// (9 a + 3 b + 3 c + d + 8) >> 4 per channel: a = S(x', y'), b = S(xn, y'), c = S(x', yn), d = S(xn, yn)
CRY_HD BloomRgb bloom_blend(BloomTexel a, BloomTexel b, BloomTexel c, BloomTexel d)
{
    BloomRgb o;
    o.r = (9u * (a[0] & 0xFFFFu) + 3u * ((b[0] & 0xFFFFu) + (c[0] & 0xFFFFu)) + (d[0] & 0xFFFFu) + 8u) >> 4;
    o.g = (9u * (a[0] >> 16) + 3u * ((b[0] >> 16) + (c[0] >> 16)) + (d[0] >> 16) + 8u) >> 4;
    o.b = (9u * a[1] + 3u * (b[1] + c[1]) + d[1] + 8u) >> 4;
    return o;
}
CRY_HD BloomRgb bloom_up(const BloomTexel* S, uint32_t sw, uint32_t sh, uint32_t x, uint32_t y)
{
    const uint32_t xc = x >> 1, xn = bloom_neighbour(x, sw);
    const uint32_t rc = (y >> 1) * sw, rn = bloom_neighbour(y, sh) * sw;
    return bloom_blend(S[rc + xc], S[rc + xn], S[rn + xc], S[rn + xn]);
}

// ---- unwind ---------------------------------------------------------------------------------------------------------------------
struct BloomUnwindArgs {
    BloomTexel* level;              // D_k in, U_k out
    const BloomTexel* upper;        // U_(k+1)
    uint32_t w, h, uw, uh, r, n;    // n = w h
};
inline BloomUnwindArgs bloom_unwind_args(void* level, const void* upper, uint32_t w, uint32_t h, uint32_t r)
{
    BloomUnwindArgs a;
    a.level = static_cast<BloomTexel*>(level);
    a.upper = static_cast<const BloomTexel*>(upper);
    a.w = w; a.h = h; a.uw = (w + 1u) >> 1; a.uh = (h + 1u) >> 1; a.r = r; a.n = w * h;
    return a;
}
CRY_HD void bloom_unwind(const BloomUnwindArgs& a, uint32_t i)
{
    if (i >= a.n) return;
    const uint32_t y = i / a.w, x = i - y * a.w;
    const BloomRgb u = bloom_up(a.upper, a.uw, a.uh, x, y);
    const BloomTexel d = a.level[i];
    const uint32_t keep = 256u - a.r;
    const uint32_t R = ((d[0] & 0xFFFFu) * keep + u.r * a.r + 128u) >> 8;
    const uint32_t G = ((d[0] >> 16) * keep + u.g * a.r + 128u) >> 8;
    const uint32_t B = (d[1] * keep + u.b * a.r + 128u) >> 8;
    a.level[i] = BloomTexel{ R | (G << 16), B };
}

// ---- composite ------------------------------------------------------------------------------------------------------------------
struct BloomCompositeArgs {
    const uint32_t* in;
    uint32_t* out;
    const BloomTexel* u1;
    uint32_t W, uw, uh, p0, p1, first, I, vec, inPlace;     // pixels [p0, p1) of the plane as one line; first: the first group or pixel
};
struct BloomCompositeLaunch { BloomCompositeArgs args; uint32_t groups; };

inline BloomCompositeLaunch bloom_composite_launch(const uint8_t* in, uint8_t* out, const void* u1, uint32_t W, uint32_t H, uint32_t row0,
                                                   uint32_t rows, uint32_t intensity)
{
    BloomCompositeLaunch L;
    BloomCompositeArgs& a = L.args;
    a.in = reinterpret_cast<const uint32_t*>(in);
    a.out = reinterpret_cast<uint32_t*>(out);
    a.u1 = static_cast<const BloomTexel*>(u1);
    a.W = W; a.uw = (W + 1u) >> 1; a.uh = (H + 1u) >> 1;
    a.p0 = row0 * W; a.p1 = (row0 + rows) * W;
    a.I = intensity;
    a.inPlace = in == out ? 1u : 0u;
    a.vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0u ? 1u : 0u;
    // vec: thread i owns pixels 4 (first + i) .. + 3, the groups that meet [p0, p1); else thread i owns pixel first + i
    a.first = a.vec ? a.p0 >> 2 : a.p0;
    const uint32_t items = rows == 0u ? 0u : (a.vec ? ((a.p1 + 3u) >> 2) - a.first : a.p1 - a.p0);
    L.groups = (items + kBloomThreads - 1u) / kBloomThreads;
    return L;
}

CRY_HD uint32_t bloom_add(uint32_t px, BloomRgb up, uint32_t I, uint32_t& added)
{
    const uint32_t ar = (up.r * I + 32768u) >> 16, ag = (up.g * I + 32768u) >> 16, ab = (up.b * I + 32768u) >> 16;
    added |= ar | ag | ab;
    uint32_t R = (px & 255u) + ar, G = ((px >> 8) & 255u) + ag, B = ((px >> 16) & 255u) + ab;
    R = R < 255u ? R : 255u; G = G < 255u ? G : 255u; B = B < 255u ? B : 255u;
    return R | (G << 8) | (B << 16) | (px & 0xFF000000u);
}

// What thread i of the launch holds between its two phases: up to four pixels and which of them it owns.
struct BloomCompositeLane { BloomQuad px; uint32_t base, mask, added; };

// Phase 1, thread i of the whole launch: loads and computes its pixels.  lane.added == 0: nothing was added to any of them.
CRY_HD BloomCompositeLane bloom_composite_eval(const BloomCompositeArgs& a, uint32_t i)
{
    BloomCompositeLane l;
    l.px = BloomQuad{ 0u, 0u, 0u, 0u };
    l.mask = 0u; l.added = 0u;
    if (!a.vec) {
        l.base = a.first + i;
        if (l.base >= a.p1 || l.base < a.first) return l;
        const uint32_t y = l.base / a.W, x = l.base - y * a.W;
        l.px[0] = bloom_add(a.in[l.base], bloom_up(a.u1, a.uw, a.uh, x, y), a.I, l.added);
        l.mask = 1u;
        return l;
    }
    const uint32_t g = a.first + i;
    l.base = g << 2;
    if (g < a.first || g > (a.p1 - 1u) >> 2) return l;        // p1 > p0 >= 0: the launch has no thread for rows == 0
    for (uint32_t c = 0; c < 4u; ++c)
        if (l.base + c >= a.p0 && l.base + c < a.p1) l.mask |= 1u << c;
    const uint32_t y = l.base / a.W, x = l.base - y * a.W;
    if (l.mask == 15u && !(x & 1u) && x + 3u < a.W) {
        // four pixels of one row from an even column: x' is c0, c0, c0 + 1, c0 + 1 and xn is c0 - 1, c0 + 1, c0, c0 + 2, so the
        // eight texels of columns c0 - 1 .. c0 + 2 (clamped) in rows y' and yn serve all four
        l.px = *reinterpret_cast<const BloomQuad*>(a.in + l.base);
        const uint32_t c0 = x >> 1, c1 = c0 + 1u;               // c1 = (x + 2) >> 1 <= (W - 1) >> 1 = uw - 1
        const uint32_t cl = c0 ? c0 - 1u : 0u, cr = c1 + 1u < a.uw ? c1 + 1u : a.uw - 1u;
        const BloomTexel* rc = a.u1 + (y >> 1) * a.uw;
        const BloomTexel* rn = a.u1 + bloom_neighbour(y, a.uh) * a.uw;
        const BloomTexel tl = rc[cl], t0 = rc[c0], t1 = rc[c1], tr = rc[cr];
        const BloomTexel nl = rn[cl], n0 = rn[c0], n1 = rn[c1], nr = rn[cr];
        l.px[0] = bloom_add(l.px[0], bloom_blend(t0, tl, n0, nl), a.I, l.added);
        l.px[1] = bloom_add(l.px[1], bloom_blend(t0, t1, n0, n1), a.I, l.added);
        l.px[2] = bloom_add(l.px[2], bloom_blend(t1, t0, n1, n0), a.I, l.added);
        l.px[3] = bloom_add(l.px[3], bloom_blend(t1, tr, n1, nr), a.I, l.added);
        return l;
    }
    uint32_t px = x, py = y;
    for (uint32_t c = 0; c < 4u; ++c) {
        if (l.mask & (1u << c)) l.px[c] = bloom_add(a.in[l.base + c], bloom_up(a.u1, a.uw, a.uh, px, py), a.I, l.added);
        if (++px == a.W) { px = 0u; ++py; }
    }
    return l;
}

// Phase 2: the stores.  The caller skips it for a wavefront of an in-place call in which no lane added anything.
CRY_HD void bloom_composite_store(const BloomCompositeArgs& a, const BloomCompositeLane& l)
{
    if (l.mask == 15u) {
        *reinterpret_cast<BloomQuad*>(a.out + l.base) = l.px;
        return;
    }
    for (uint32_t c = 0; c < 4u; ++c)
        if (l.mask & (1u << c)) a.out[l.base + c] = l.px[c];
}

}  // namespace cry
