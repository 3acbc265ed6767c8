// post_aa_core.hpp -- the per-tile body of crychic_antialias (post_aa.hip), written so that a host compiler
// builds it too (tests/post_aa_host): one call per thread and phase, the caller supplies the barriers between the phases and the
// wave vote.
//
// Definition (include/crychic_hip.h): an FXAA-class pass over a finished RGBA8 frame, in 32-bit integers throughout.  Per pixel:
// luma range of the cross neighbourhood against a threshold (below it: copy), edge orientation from the 3 x 3 lumas, the side
// across the edge with the steeper gradient, a search of up to K steps along the edge in both directions for its ends, an edge
// weight from the nearer end, a sub-pixel weight from the 3 x 3 low-pass, and a blend with the across-neighbour by the larger.
//
// Structure: one workgroup of 256 threads per 64 x 32 output tile.  Phase 1 (post_aa_fill) loads the tile with an apron of
// kAaApron = CRYCHIC_AA_MAX_SEARCH texels on every side -- 24 x 64 quads of four texels, six per thread -- and leaves each texel's
// luma in LDS as a uint16 (96 x 64 x 2 B = 12 KiB): a luma is computed once, not once per 3 x 3 tap and search step.  Coordinates
// clamp at fill time, so an LDS position outside the frame holds the luma of the nearest texel inside and the later phases address LDS by
// plain offsets: +-16 along either axis and +-1 across never leaves the 96 x 64 array.  A thread's two own quads (rows t / 16 and
// t / 16 + 16 of the tile, columns 4 (t % 16) ..) are among the six it loads: their colours stay in registers as the centre
// colours.  Phase 2 (post_aa_detect) runs step 1 per texel of those quads: a texel below the threshold is stored at once, an edge texel
// goes onto a list in LDS.  Phase 3 (post_aa_edges) runs steps 2 .. 7 over the list, one texel per lane: edge texels are few and lie
// along lines, so in the quads' own layout a wavefront would run the long edge path with a handful of lanes active, once per texel
// slot; from the list the lanes are dense.  The centre and the across-neighbour colour of an edge texel are two dwords read back from
// global memory.  `any` is the wave vote that ends the search loop when every lane that searches has found both ends; results never
// depend on it (a host build passes the lane's own predicate).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if !defined(CRY_HD)                // devmath.hpp's definition; this header stands alone so that any host compiler builds it
#if defined(__HIPCC__)
#define CRY_HD __host__ __device__ __forceinline__
#else
#define CRY_HD inline
#endif
#endif

namespace cry {

constexpr uint32_t kAaMaxSearch = 16u;              // CRYCHIC_AA_MAX_SEARCH (api.cpp asserts the two agree)
constexpr uint32_t kAaTileW = 64u, kAaTileH = 32u;  // output texels per workgroup
constexpr uint32_t kAaThreads = 256u;
constexpr uint32_t kAaApron = kAaMaxSearch;
constexpr uint32_t kAaLdsW = kAaTileW + 2u * kAaApron;      // 96
constexpr uint32_t kAaLdsH = kAaTileH + 2u * kAaApron;      // 64
constexpr uint32_t kAaLdsTexels = kAaLdsW * kAaLdsH;        // uint16 each
constexpr uint32_t kAaQuadsPerRow = kAaLdsW / 4u;           // 24

struct PostAaParams { uint32_t absMin, relShift, searchSteps, subpix; };

// One call: rows [row0, rowEnd) of `out` from `in`, both W x H; [yLo, yHi] are the rows of `in` the call may read
// ([row0 - 16, rowEnd + 16) cut to the frame): a row coordinate clamps to them, which for the rows a written texel can reach is the
// clamp to the frame.
struct PostAaArgs {
    const uint32_t* in;
    uint32_t* out;
    uint32_t W, H, row0, rowEnd, yLo, yHi;
    PostAaParams p;
};

// Native 16-byte vector for the aligned loads and stores of four texels, and the 8 bytes of four lumas in LDS.
typedef uint32_t PostAaTexels4 __attribute__((ext_vector_type(4)));
typedef uint32_t PostAaLumas4 __attribute__((ext_vector_type(2), may_alias, aligned(8)));

// What a thread carries from phase 1 to phase 2: the colours of its two quads.
struct PostAaLane { PostAaTexels4 c[2]; };

CRY_HD uint32_t post_aa_luma(uint32_t texel) { return 77u * (texel & 255u) + 150u * ((texel >> 8) & 255u) + 29u * ((texel >> 16) & 255u); }
CRY_HD int32_t post_aa_abs(int32_t v) { return v < 0 ? -v : v; }
CRY_HD int32_t post_aa_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Texels xs .. xs + 3 of row y, each column clamped to the frame.  VEC: W is a multiple of 4, the plane 16-byte aligned and xs a
// multiple of 4, so the quad lies wholly inside the frame or wholly outside it -- one 16-byte load of the nearest quad inside, and
// outside the frame its edge texel four times.  Otherwise four dword loads.  A template parameter, so that the two paths are two
// kernels (cube_mips_core.hpp).
template <bool VEC>
CRY_HD PostAaTexels4 post_aa_load_quad(const uint32_t* in, uint32_t W, int32_t xs, uint32_t y)
{
    const uint32_t* row = in + (size_t)y * W;
    PostAaTexels4 v;
    if (VEC) {
        const int32_t xq = xs < 0 ? 0 : (xs >= (int32_t)W ? (int32_t)W - 4 : xs);
        v = *reinterpret_cast<const PostAaTexels4*>(row + xq);
        if (xs < 0) v = PostAaTexels4{ v[0], v[0], v[0], v[0] };
        else if (xs >= (int32_t)W) v = PostAaTexels4{ v[3], v[3], v[3], v[3] };
    } else {
        for (int32_t i = 0; i < 4; ++i) v[i] = row[post_aa_clamp(xs + i, 0, (int32_t)W - 1)];
    }
    return v;
}

// LDS quad (q, r) of the six a thread fills: k = 0, 1 are its own quads, k = 2 .. 5 its share of the 1024 apron quads (384 above the
// tile, 384 below, 128 to each side).
CRY_HD void post_aa_fill_slot(uint32_t t, uint32_t k, uint32_t& q, uint32_t& r)
{
    if (k < 2u) {
        q = kAaApron / 4u + (t & 15u);
        r = kAaApron + (t >> 4) + 16u * k;
        return;
    }
    const uint32_t j = t + kAaThreads * (k - 2u);                   // 0 .. 1023
    const uint32_t band = kAaApron * kAaQuadsPerRow;                // 384
    if (j < band) { r = j / kAaQuadsPerRow; q = j % kAaQuadsPerRow; }
    else if (j < 2u * band) { r = kAaApron + kAaTileH + (j - band) / kAaQuadsPerRow; q = (j - band) % kAaQuadsPerRow; }
    else {
        const uint32_t s = j - 2u * band;                           // 0 .. 255: 32 rows of four quads left and four right
        r = kAaApron + s / 8u;
        q = (s & 7u) < 4u ? (s & 7u) : (s & 7u) + kAaTileW / 4u;
    }
}

// Phase 1, thread t of 256 of tile (tileX, tileY): its six quads -> lumas in `tile`; the colours of its own two -> lane.
template <bool VEC>
CRY_HD void post_aa_fill(const PostAaArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, uint16_t* tile, PostAaLane& lane)
{
    const int32_t x0 = (int32_t)(tileX * kAaTileW) - (int32_t)kAaApron;
    const int32_t y0 = (int32_t)(a.row0 + tileY * kAaTileH) - (int32_t)kAaApron;
    PostAaTexels4 v[6];
    uint32_t at[6];
    for (uint32_t k = 0; k < 6u; ++k) {
        uint32_t q, r;
        post_aa_fill_slot(t, k, q, r);
        at[k] = r * kAaLdsW + 4u * q;
        v[k] = post_aa_load_quad<VEC>(a.in, a.W, x0 + (int32_t)(4u * q), (uint32_t)post_aa_clamp(y0 + (int32_t)r, (int32_t)a.yLo, (int32_t)a.yHi));
    }
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);          // all of a thread's loads before any of the arithmetic that waits for them
#endif
    for (uint32_t k = 0; k < 6u; ++k) {
        PostAaLumas4 l;
        l[0] = post_aa_luma(v[k][0]) | (post_aa_luma(v[k][1]) << 16);
        l[1] = post_aa_luma(v[k][2]) | (post_aa_luma(v[k][3]) << 16);
        *reinterpret_cast<PostAaLumas4*>(tile + at[k]) = l;
    }
    lane.c[0] = v[0];
    lane.c[1] = v[1];
}

// c blended towards n by w of 256, channel by channel with rounding; two channels per multiply (a product plus 128 is at most
// 255 * 256 + 128 and never carries into its neighbour).
CRY_HD uint32_t post_aa_blend(uint32_t c, uint32_t n, uint32_t w)
{
    const uint32_t m = 0x00FF00FFu;
    const uint32_t rb = (c & m) * (256u - w) + (n & m) * w + 0x00800080u;
    const uint32_t ga = ((c >> 8) & m) * (256u - w) + ((n >> 8) & m) * w + 0x00800080u;
    return ((rb >> 8) & m) | (ga & ~m);
}

// Steps 2 .. 7 of one edge texel.  n: the 3 x 3 lumas (rows N, M, S); at: the texel's offset in `tile`; (x, y): its frame
// coordinates; range: step 1's.  Returns the blended colour of centre colour c.
template <typename Any>
CRY_HD uint32_t post_aa_edge_texel(const PostAaArgs& a, const uint16_t* tile, int32_t at, const int32_t (&n)[3][3], int32_t range, uint32_t x,
                                   uint32_t y, uint32_t c, Any any)
{
    const int32_t NW = n[0][0], N = n[0][1], NE = n[0][2], Wl = n[1][0], M = n[1][1], E = n[1][2], SW = n[2][0], S = n[2][1], SE = n[2][2];
    // 2: orientation
    const int32_t horz = post_aa_abs(NW - 2 * Wl + SW) + 2 * post_aa_abs(N - 2 * M + S) + post_aa_abs(NE - 2 * E + SE);
    const int32_t vert = post_aa_abs(NW - 2 * N + NE) + 2 * post_aa_abs(Wl - 2 * M + E) + post_aa_abs(SW - 2 * S + SE);
    const bool horizontal = horz >= vert;
    // 3: the side across the edge
    const int32_t la = horizontal ? N : Wl, lb = horizontal ? S : E;
    const int32_t gA = post_aa_abs(la - M), gB = post_aa_abs(lb - M);
    const bool sideA = gA >= gB;
    const int32_t g = sideA ? gA : gB, nb = sideA ? la : lb;
    const int32_t Lp = M + nb;
    // 4: the ends, both directions in one loop
    const int32_t along = horizontal ? 1 : (int32_t)kAaLdsW;
    const int32_t across = (sideA ? -1 : 1) * (horizontal ? (int32_t)kAaLdsW : 1);
    const int32_t K = (int32_t)(a.p.searchSteps < kAaMaxSearch ? a.p.searchSteps : kAaMaxSearch);     // the apron bounds the reach
    int32_t dn = K, dp = K, en = 0, ep = 0;
    bool doneN = false, doneP = false;
    for (int32_t i = 1; i <= K; ++i) {
        const int32_t qn = at - i * along, qp = at + i * along;
        const int32_t d0 = (int32_t)tile[qn] + (int32_t)tile[qn + across] - Lp;
        const int32_t d1 = (int32_t)tile[qp] + (int32_t)tile[qp + across] - Lp;
        if (!doneN) {
            en = d0;
            if (2 * post_aa_abs(d0) >= g) { doneN = true; dn = i; }
        }
        if (!doneP) {
            ep = d1;
            if (2 * post_aa_abs(d1) >= g) { doneP = true; dp = i; }
        }
        if (!any(!(doneN && doneP))) break;
    }
    // 5: edge weight
    const int32_t dmin = dn <= dp ? dn : dp, e = dn <= dp ? en : ep;
    const int32_t wE = ((e < 0) != (M - nb < 0)) ? 128 - (256 * dmin) / (dn + dp) : 0;
    // 6: sub-pixel weight
    const int32_t s = 2 * (N + S + E + Wl) + NW + NE + SW + SE;
    const uint32_t tt = (uint32_t)post_aa_abs(s - 12 * M);
    uint32_t r = (256u * tt) / (12u * (uint32_t)range);
    r = r < 256u ? r : 256u;
    const uint32_t r2 = (r * r * (768u - 2u * r)) >> 16;
    const int32_t wS = (int32_t)((((r2 * r2) >> 8) * a.p.subpix) >> 8);
    // 7: blend with the across-neighbour, read back from the frame
    const int32_t w = wE > wS ? wE : wS;
    const int32_t step = sideA ? -1 : 1;
    const int32_t nx = horizontal ? (int32_t)x : post_aa_clamp((int32_t)x + step, 0, (int32_t)a.W - 1);
    const int32_t ny = horizontal ? post_aa_clamp((int32_t)y + step, 0, (int32_t)a.H - 1) : (int32_t)y;
    return post_aa_blend(c, a.in[(size_t)ny * a.W + (uint32_t)nx], (uint32_t)w);
}

// The edge texels of a tile, found in phase 2 and resolved in phase 3: count, then tile-local positions ty * 64 + tx in any order.
struct PostAaEdgeList { uint32_t count; uint16_t at[kAaTileW * kAaTileH]; };

CRY_HD uint32_t post_aa_append(uint32_t* count)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(count, 1u);
#else
    return (*count)++;              // the host build runs the threads of a phase one after the other
#endif
}

// Phase 2, thread t: step 1 for the texels of its two quads, from the lumas in `tile` (complete: the caller's barrier) and the colours
// in `lane`.  A texel below the threshold is stored as it is -- a whole quad of them in one store; an edge texel is not stored here but
// appended to `list`.
template <bool VEC>
CRY_HD void post_aa_detect(const PostAaArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, const uint16_t* tile, const PostAaLane& lane,
                           PostAaEdgeList* list)
{
    const uint32_t cx = t & 15u, ry = t >> 4;
    const uint32_t x = tileX * kAaTileW + 4u * cx;
    for (uint32_t p = 0; p < 2u; ++p) {
        const uint32_t ty = ry + 16u * p, y = a.row0 + tileY * kAaTileH + ty;
        if (y >= a.rowEnd) continue;
        const int32_t at = (int32_t)((kAaApron + ty) * kAaLdsW + kAaApron + 4u * cx);
        int32_t l[3][6];                                    // lumas of rows y - 1 .. y + 1, columns x - 1 .. x + 4
        for (int32_t j = 0; j < 3; ++j) {
            const uint16_t* row = tile + at + (j - 1) * (int32_t)kAaLdsW;
            const PostAaLumas4 m = *reinterpret_cast<const PostAaLumas4*>(row);
            l[j][0] = row[-1];
            l[j][1] = (int32_t)(m[0] & 0xFFFFu); l[j][2] = (int32_t)(m[0] >> 16);
            l[j][3] = (int32_t)(m[1] & 0xFFFFu); l[j][4] = (int32_t)(m[1] >> 16);
            l[j][5] = row[4];
        }
        bool edge[4];
        for (uint32_t i = 0; i < 4u; ++i) {
            const int32_t N = l[0][i + 1], Wl = l[1][i], M = l[1][i + 1], E = l[1][i + 2], S = l[2][i + 1];
            int32_t hi = M, lo = M;
            hi = N > hi ? N : hi; hi = S > hi ? S : hi; hi = E > hi ? E : hi; hi = Wl > hi ? Wl : hi;
            lo = N < lo ? N : lo; lo = S < lo ? S : lo; lo = E < lo ? E : lo; lo = Wl < lo ? Wl : lo;
            const uint32_t range = (uint32_t)(hi - lo), rel = (uint32_t)hi >> a.p.relShift;
            edge[i] = x + i < a.W && range != 0u && range >= (a.p.absMin > rel ? a.p.absMin : rel);
            if (edge[i]) list->at[post_aa_append(&list->count)] = (uint16_t)(ty * kAaTileW + 4u * cx + i);
        }
        uint32_t* dst = a.out + (size_t)y * a.W + x;
        if (VEC && !(edge[0] || edge[1] || edge[2] || edge[3])) {           // W is a multiple of 4: the whole quad or none of it
            if (x < a.W) *reinterpret_cast<PostAaTexels4*>(dst) = lane.c[p];
        } else {
            for (uint32_t i = 0; i < 4u; ++i)
                if (x + i < a.W && !edge[i]) dst[i] = lane.c[p][i];
        }
    }
}

// Phase 3, thread t: every 256th edge texel of `list` (complete: the caller's barrier) through steps 2 .. 7.  The texels of a tile are
// dense across the lanes here whatever their layout in the frame; centre and across-neighbour colours are read back from the frame.
template <typename Any>
CRY_HD void post_aa_edges(const PostAaArgs& a, uint32_t tileX, uint32_t tileY, uint32_t t, const uint16_t* tile, const PostAaEdgeList* list, Any any)
{
    const uint32_t count = list->count < kAaTileW * kAaTileH ? list->count : kAaTileW * kAaTileH;
    for (uint32_t k = t; k < count; k += kAaThreads) {
        const uint32_t e = list->at[k], tx = e % kAaTileW, ty = e / kAaTileW;
        const uint32_t x = tileX * kAaTileW + tx, y = a.row0 + tileY * kAaTileH + ty;
        const int32_t at = (int32_t)((kAaApron + ty) * kAaLdsW + kAaApron + tx);
        int32_t n[3][3];
        for (int32_t j = 0; j < 3; ++j)
            for (int32_t i = 0; i < 3; ++i) n[j][i] = tile[at + (j - 1) * (int32_t)kAaLdsW + (i - 1)];
        int32_t hi = n[1][1], lo = n[1][1];
        const int32_t cross[4] = { n[0][1], n[2][1], n[1][0], n[1][2] };
        for (int32_t i = 0; i < 4; ++i) { hi = cross[i] > hi ? cross[i] : hi; lo = cross[i] < lo ? cross[i] : lo; }
        const size_t px = (size_t)y * a.W + x;
        a.out[px] = post_aa_edge_texel(a, tile, at, n, hi - lo, x, y, a.in[px], any);
    }
}

// The launch plan (post_aa.hip's launcher and the host harness walk it): the grid of tiles over rows [row0, row0 + rows), anchored
// at row0, and the 16-byte path's condition.
struct PostAaLaunch { PostAaArgs args; uint32_t tilesX, tilesY; bool vec; };
CRY_HD PostAaLaunch post_aa_launch(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const PostAaParams& p)
{
    PostAaLaunch L;
    L.args.in = reinterpret_cast<const uint32_t*>(in);
    L.args.out = reinterpret_cast<uint32_t*>(out);
    L.args.W = W; L.args.H = H; L.args.row0 = row0; L.args.rowEnd = row0 + rows;
    L.args.yLo = row0 > kAaApron ? row0 - kAaApron : 0u;
    L.args.yHi = (row0 + rows + kAaApron < H ? row0 + rows + kAaApron : H) - 1u;
    L.args.p = p;
    L.tilesX = (W + kAaTileW - 1u) / kAaTileW;
    L.tilesY = (rows + kAaTileH - 1u) / kAaTileH;
    L.vec = W % 4u == 0u && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0u;
    return L;
}

}  // namespace cry
