// kernels.hip -- gfx950 kernels of the CRYCHIC hot path and their stream-ordered launchers.
//
// Work decomposition (all kernels): one lane per output pixel, 64 consecutive pixels of one row per
// wavefront so every plane access is a contiguous 64-lane burst (16 B/lane on the fp32 G-buffer planes,
// 8 B/lane on the fp16 normal plane and the depth row pairs), 4 rows per 256-thread workgroup.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>
#include "kernels.hpp"
#include "ssao_core.hpp"
#include "blur_tiles.hpp"
#include "light_core.hpp"
#include "light_bind.hpp"
#include "light_tiles.hpp"
#include "dispatch_order.hpp"

namespace cry {

// Two-dimensional variant for the SSAO pass: the (padded) grid is cut into super-tiles of SX x SY workgroup tiles; whole
// super-tiles are dealt to the XCDs, so the depth texels an XCD's taps reach form a compact block instead of a
// full-width stripe (at 7680 x 4320 a stripe of the depth plane no longer fits the 4 MiB L2).  gridDim is a multiple of
// (SX, SY); tiles outside the frame exit at once.
__device__ __forceinline__ void tile_origin_2d(uint32_t& bx, uint32_t& by, uint32_t SX, uint32_t SY)
{
    const uint32_t ncx = gridDim.x / SX, T = SX * SY, nst = ncx * (gridDim.y / SY);
    const uint32_t b = blockIdx.y * gridDim.x + blockIdx.x;
    const uint32_t full = (nst & ~7u) * T;                // workgroups in whole groups of eight super-tiles
    uint32_t st, o;
    if (b < full) {
        const uint32_t xcd = b & 7u, k = b >> 3;          // k-th workgroup this XCD receives
        const uint32_t j = k / T;
        o = k - j * T;
        st = j * 8u + xcd;
    } else {                                              // the tail keeps its order (bijective)
        st = b / T;
        o = b - st * T;
    }
    const uint32_t sty = st / ncx, stx = st - sty * ncx, oy = o / SX, ox = o - oy * SX;
    // which XCD a super-tile goes to is settled above; its row of the frame follows the band order of dispatch_order.hpp
    // (measured best: bottom-up, so that a launch over ground under a sky ends on the short sky wavefronts)
    bx = stx * SX + ox;
    by = launch_band(sty, gridDim.y / SY, CRY_SSAO_BAND_WAYS) * SY + oy;
}

// ---- SSAO ------------------------------------------------------------------------------------------------
// Re-lays the D24 depth plane as decoded {d(x, y), d(x, y+1)} entries with a BORDER guard band (ssao_core.hpp "depth pairs").
// One wavefront per 8 entry rows x 128 entry columns: a lane owns two horizontally adjacent entries of each of the 8 rows (one
// 16-byte store per row) and reads the 9 texel rows they are built from once (one 8-byte load per row).  Entry rows are
// py = 8 cy .. 8 cy + 7 of cell row cy (texel rows py - 2 .. py - 1), entry columns 128 seg .. 128 seg + 127 of segment seg.
// By-products, both without LDS or barriers:
//   * the nearest-depth map of the tap culling: cell (cx, cy) = smallest decoded texel of padded texels [8 cx, 8 cx + 8] x
//     [8 cy, 8 cy + 8] -- the 9 rows a lane holds, over the 4 lanes of the cell plus the first column of the next lane (the last
//     cell of a wavefront takes that column from one extra load); positions outside the plane count as the clear depth, which
//     is what a footprint reaching them reads;
//   * the coarse geometry map of the sky shortcut: a wavefront covers texel columns [128 seg - 2, 128 seg + 126) of its rows; if
//     any texel of rows belonging to cell row c lies below the clear depth it stamps cell (seg, c) with this frame's stamp -- a
//     plain store: every writer of a cell stores the same value, and a stale or uninitialised word can only read as "geometry"
//     (no shortcut), never as "sky".
template <bool WRITE_PAIRS>
__global__ __launch_bounds__(256) void depth_pairs_kernel(const uint32_t* __restrict__ depth, f4a* __restrict__ pairs, uint32_t* __restrict__ geo,
                                                          float* __restrict__ zcull, uint32_t stamp, uint32_t W, uint32_t H, CullParams cull,
                                                          uint32_t cellRow0)
{
    const uint32_t halfPitch = depth_pairs_pitch(W) / 2u;
    const uint32_t lane = threadIdx.x & 63u, seg = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (seg * 64u >= halfPitch) return;                          // wave-uniform
    const uint32_t px2 = seg * 64u + lane, cy = cellRow0 + blockIdx.y;
    const int x = 2 * (int)px2 - 2, y0 = 8 * (int)cy - 2;         // first texel column of the lane, first texel row of the wave
    const bool inx = (uint32_t)x < W;                             // W even, x even: x + 1 < W as well
    const uint32_t cx = inx ? (uint32_t)x : 0u;
    float r0[9], r1[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int y = y0 + k;
        RawPair t{ 0x00FFFFFFu, 0x00FFFFFFu };
        if (inx && (uint32_t)y < H) t = load_at<RawPair>(depth, (mul24((uint32_t)y, W) + cx) * 4u);
        r0[k] = d24_to_float(t.lo);
        r1[k] = d24_to_float(t.hi);
    }
    const bool live = px2 < halfPitch;
    // coarse geometry map: rows y0 .. y0 + 7 (row y0 + 8 is the next cell row's first) fall into at most two 32-row cells
    const int yFirst = y0 < 0 ? 0 : y0;
    const uint32_t c0 = (uint32_t)yFirst >> 5;
    bool geoA = false, geoB = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int y = y0 + k;
        const bool g = (r0[k] != 1.0f) | (r1[k] != 1.0f);          // BORDER and clear-depth texels decode to 1.0
        if ((uint32_t)y < H) { if (((uint32_t)y >> 5) == c0) geoA |= g; else geoB |= g; }
    }
    const bool anyA = __builtin_amdgcn_ballot_w64(geoA) != 0, anyB = __builtin_amdgcn_ballot_w64(geoB) != 0;
    if (lane == 0) {
        if (anyA) geo[c0 * geo_map_cols(W) + seg] = stamp;
        if (anyB) geo[(c0 + 1u) * geo_map_cols(W) + seg] = stamp;
    }
    // nearest-depth map
    float mFirst = r0[0], mSecond = r1[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) { mFirst = __builtin_fminf(mFirst, r0[k]); mSecond = __builtin_fminf(mSecond, r1[k]); }
    float m = __builtin_fminf(mFirst, mSecond);
    m = __builtin_fminf(m, __shfl_xor(m, 1));
    m = __builtin_fminf(m, __shfl_xor(m, 2));                       // the cell's own 8 columns
    float next = __shfl(mFirst, (int)((lane | 3u) + 1u) & 63);      // first column of the next cell (lanes 60..63: replaced below)
    {
        // column 128 seg + 126 (texel), rows y0 .. y0 + 8: lanes 0 .. 8 load one texel each
        const int xe = 128 * (int)seg + 126, ye = y0 + (int)lane;
        float v = 1.0f;
        if (lane < 9u && (uint32_t)xe < W && (uint32_t)ye < H) v = d24_to_float(load_at<uint32_t>(depth, (mul24((uint32_t)ye, W) + (uint32_t)xe) * 4u));
        v = __builtin_fminf(v, __shfl_xor(v, 1));
        v = __builtin_fminf(v, __shfl_xor(v, 2));
        v = __builtin_fminf(v, __shfl_xor(v, 4));
        v = __builtin_fminf(v, __shfl_xor(v, 8));
        v = __shfl(v, 0);
        if (lane >= 60u) next = v;
    }
    m = __builtin_fminf(m, next);                                   // the same value in the four lanes of a cell
    // The pairs plane.  A lane's entries (2 px2, 2 px2 + 1) are read by footprints whose left entry is 2 px2 - 1, 2 px2 or 2 px2 + 1:
    // its own cell, and for the first lane of a cell the cell to the left as well.  Entries that only clear cells can reach are
    // read by nobody (ssao_core.hpp "clear cells") and are not written.  The first cell of a wavefront always writes: its left
    // neighbour belongs to another wavefront.
    const float left = __shfl(m, (int)(lane - 1u) & 63);
    const bool unread = cull.clear && m == 1.0f && lane >= 4u && ((lane & 3u) != 0u || left == 1.0f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t py = 8u * cy + (uint32_t)k;
        if (WRITE_PAIRS && live && !unread && py < H + 3u) pairs[py * halfPitch + px2] = f4a{ r0[k], r0[k + 1], r1[k], r1[k + 1] };
    }
    const uint32_t cellX = seg * 16u + (lane >> 2);
    if ((lane & 3u) == 0 && cellX < zmin_map_cols(W)) zcull[cy * zmin_map_cols(W) + cellX] = zmin_cell_value(cull, m);
}

// Shaders/Ssao.hlsl:117-199 over half-res rows [row0, row1).  EMIT_AO = false builds only the edge workspace.
// PAIRS: the depth taps read the pairs plane of the edge workspace (built by depth_pairs_kernel earlier on the stream).
// MAPS: the depth pass of this frame built the coarse maps (geometry, nearest depth) that the sky shortcut and the tap culling read.
// ROWS: that pass was limited to the footprint rows [prepJ0, prepJ0 + prepNj) (a strip of a multi-GPU frame): taps that leave them
// gather from the raw plane (ssao_core.hpp DepthPairsRows).
struct PrepRows { int j0lo; uint32_t nj; };
template <bool EMIT_AO, bool PAIRS, bool MAPS, bool ROWS>
__global__ __launch_bounds__(256) void ssao_kernel(crychic_ssao_constants cb, const u2* __restrict__ normal,
                                                   const uint32_t* __restrict__ depth,
                                                   const uint32_t* __restrict__ randvec,
                                                   uint16_t* __restrict__ ambient, EdgePlane edge, uint32_t W,
                                                   uint32_t H, uint32_t row0, uint32_t row1, uint32_t SX, uint32_t SY, int sparseProjTex,
                                                   SkyReach sky, uint32_t stamp, int cullEnabled, PrepRows prep, HalfResScale hs)
{
    const uint32_t w2 = W / 2;
    uint32_t bx, by;
    tile_origin_2d(bx, by, SX, SY);
    const uint32_t x = bx * 64u + (threadIdx.x & 63u);
    const uint32_t y = row0 + by * 4u + (threadIdx.x >> 6);
    if (x >= w2 || y >= row1) return;

    const DepthPairs dp{ edge.pairs, depth_pairs_pitch(W) };
    const DepthD24 dd{ depth, W, H };
    // ---- the wavefront's one batch of loads: nothing in it waits for anything else in it ----
    // the pixel's own depth comes from the D24 plane (coalesced): its pairs entry may be one the depth pass did not write
    const SsaoCentreRaw cr = ssao_centre_fetch(normal, depth, W, H, (int)x, (int)y);
    // the random-vector texels of the tap loop: their addresses depend on (x, y) alone
    RandvecRaw rv{};
    if (EMIT_AO) rv = ssao_pixel_randvec_fetch(randvec, x, y, hs);
    // the cells of the geometry map the sky shortcut may ask for, one per lane: the rectangle depends on the wavefront's position
    // and the kernel's arguments alone, so it is addressed (on wave-uniform values: x0 and the row are the same in every lane)
    // and fetched before anyone knows whether the wavefront is sky
    const bool skyMaps = EMIT_AO && MAPS && sky.enabled;
    const uint32_t x0 = bx * 64u, n = (w2 - x0) < 64u ? (w2 - x0) : 64u;
    GeoCells g{};
    uint32_t cellWord = 0u;
    if (skyMaps) {
        g = ssao_sky_cells(sky, W, H, x0, n, (uint32_t)__builtin_amdgcn_readfirstlane((int)y));
        cellWord = edge.geo[ssao_sky_cell_of_lane(g, geo_map_cols(W), threadIdx.x & 63u)];
    }
    // the border texels of the edge workspace, under their lane predicates
    u2 gcolTexel{}, growTexel{};
    if (edge.nrm) {
        if (x == 0) gcolTexel = normal[(2u * y + 1u) * W];      // texel (0, 2y+1)
        if (y == row0) growTexel = normal[2u * x + 1u];         // texel (2x+1, 0)
    }
    // ---- the batch is in flight ----
    const SsaoCentre c = ssao_centre_resolve(cb, cr);
    if (edge.nrm) {
        const uint32_t idx = y * w2 + x;
        edge.nrm[idx] = c.nrm_bits;
        edge.vz[idx] = c.vz;
        if (x == 0) edge.gcol[y] = gcolTexel;
        if (y == row0) edge.grow[x] = growTexel;
    }
    // Sky shortcut (ssao_core.hpp): every live lane of this wave is a sky pixel and no cell its taps can reach holds geometry
    if (skyMaps && __builtin_amdgcn_ballot_w64(!c.sky) == 0) {
        const uint32_t ncx = g.cx1 - g.cx0 + 1u, ncells = ncx * (g.cy1 - g.cy0 + 1u), pitch = geo_map_cols(W);
        bool geometry = cellWord == stamp;                                    // lanes 0 .. ncells-1 hold the cells: enough when ncells <= n
        if (ncells > n) {
            // a rectangle of more cells than the wave has live lanes (more than 64 cells, or a short wave at the frame's edge
            // with a wide reach): the n live lanes (0 .. n-1) share the cells in a loop
            geometry = false;
            for (uint32_t k = threadIdx.x & 63u; k < ncells; k += n) {
                const uint32_t cy = k / ncx, cx = k - cy * ncx;
                geometry |= edge.geo[(g.cy0 + cy) * pitch + g.cx0 + cx] == stamp;
            }
        }
        if (g.known && __builtin_amdgcn_ballot_w64(geometry) == 0) {
            ambient[y * w2 + x] = (uint16_t)0xFFFFu;
            if ((threadIdx.x & 63u) == 0) edge.ones[y * ones_map_cols(W) + bx] = stamp;
            return;
        }
    }
    if (EMIT_AO) {
        uint32_t v;
        const ZminMap zm{ edge.zcull, zmin_map_cols(W) };
        if (ROWS && PAIRS) {      // && MAPS
            const DepthPairsRows dr{ dp, dd, prep.j0lo, prep.nj };
            if (cullEnabled) v = ssao_pixel_fetched(cb, c, dr, rv, W, H, x, y, hs, sparseProjTex != 0, ZminMapRows{ zm, prep.j0lo, prep.nj });
            else v = ssao_pixel_fetched(cb, c, dr, rv, W, H, x, y, hs, sparseProjTex != 0);
        }
        else if (ROWS) {          // MAPS without the pairs plane: the taps gather from the raw plane, the culling map is the strip's
            if (cullEnabled) v = ssao_pixel_fetched(cb, c, dd, rv, W, H, x, y, hs, sparseProjTex != 0, ZminMapRows{ zm, prep.j0lo, prep.nj });
            else v = ssao_pixel_fetched(cb, c, dd, rv, W, H, x, y, hs, sparseProjTex != 0);
        }
        else if (PAIRS && MAPS && cullEnabled) v = ssao_pixel_fetched(cb, c, dp, rv, W, H, x, y, hs, sparseProjTex != 0, zm);
        else if (PAIRS) v = ssao_pixel_fetched(cb, c, dp, rv, W, H, x, y, hs, sparseProjTex != 0);
        else if (MAPS && cullEnabled) v = ssao_pixel_fetched(cb, c, dd, rv, W, H, x, y, hs, sparseProjTex != 0, zm);
        else v = ssao_pixel_fetched(cb, c, dd, rv, W, H, x, y, hs, sparseProjTex != 0);
        ambient[y * w2 + x] = (uint16_t)v;
        // unoccluded-wavefront map (ssao_core.hpp "unoccluded tiles"): lane 0 is live whenever the wave is (x = 64 bx < w2).  The
        // word is written by EVERY wavefront that emits ambient values -- the stamp or 0 -- so no word of a row computed this
        // frame is ever stale.
        if (MAPS && stamp != 0u) {
            const bool allOnes = __builtin_amdgcn_ballot_w64(v != 0xFFFFu) == 0;
            if ((threadIdx.x & 63u) == 0) edge.ones[y * ones_map_cols(W) + bx] = allOnes ? stamp : 0u;
        }
    }
}

// ---- bilateral blur ------------------------------------------------------------------------------------------
// Shaders/SsaoBlur.hlsl:85-146, one self-contained sweep (crychic_ssao_blur == Ssao::BlurAmbientMap(cmdList, bool), Ssao.cpp:245-293).
// A 64 x 16 output tile plus its 5-pixel apron along the sweep axis is staged once in LDS as pre-decoded floats (normal.xyz +
// linear depth as one 16-byte entry, ambient as one dword), so the 11-tap window of every pixel is served by one ds_read_b128 +
// one ds_read_b32 per tap instead of 3 global fetches + 4 format conversions.  Consecutive lanes read consecutive 16-byte
// entries (conflict-free for both directions: the horizontal window slides along a staged row, the vertical one hops whole rows).
template <bool HORZ>
__global__ __launch_bounds__(256) void blur_kernel(crychic_ssao_constants cb, EdgePlane edge,
                                                   const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                   uint32_t W, uint32_t H, uint32_t row0, uint32_t row1)
{
    constexpr int BW = 64, BH = 16, R = 5;
    constexpr int SW = HORZ ? BW + 2 * R : BW;
    constexpr int SH = HORZ ? BH : BH + 2 * R;
    __shared__ f4a s_nz[SW * SH];
    __shared__ float s_a[SW * SH];

    const int w2 = (int)(W / 2), h2 = (int)(H / 2);
    uint32_t bx, by;
    tile_origin<4>(bx, by);
    const int x0 = (int)bx * BW, y0 = (int)row0 + (int)by * BH;
    const int sx0 = HORZ ? x0 - R : x0, sy0 = HORZ ? y0 : y0 - R;
    const float borderZ = ndc_to_view(cb, 1.0f);

    for (int k = (int)threadIdx.x; k < SW * SH; k += 256) {
        const int ly = k / SW, lx = k - ly * SW;
        const BlurTap t = blur_fetch(edge, in, borderZ, w2, h2, sx0 + lx, sy0 + ly);
        s_nz[k] = f4a{ t.n.x, t.n.y, t.n.z, t.z };
        s_a[k] = t.a;
    }
    __syncthreads();

    const int tx = (int)(threadIdx.x & 63u), tyb = (int)(threadIdx.x >> 6);
    const int x = x0 + tx;
#pragma unroll
    for (int j = 0; j < BH / 4; ++j) {
        const int ty = tyb + 4 * j;
        const int y = y0 + ty;
        if (x < w2 && y < (int)row1) {
            const uint32_t v = blur_pixel(&cb.BlurWeights[0][0], [&](int i) {
                const int idx = HORZ ? ty * SW + tx + i : (ty + i) * SW + tx;
                const f4a q = s_nz[idx];
                return BlurTap{ f3{ q.x, q.y, q.z }, q.w, s_a[idx] };
            });
            out[(uint32_t)y * (uint32_t)w2 + (uint32_t)x] = (uint16_t)v;
        }
    }
}

// The workgroup behind the tile bodies of blur_tiles.hpp.  COHERENT: the ambient planes are read and written with agent-scope
// (device-coherent) accesses -- the single-launch chain, whose tiles hand values to workgroups on other XCDs inside one kernel.
template <bool COHERENT = false>
struct BlockDevT {
    static constexpr int kLanes = 1;
    __device__ int tid() const { return (int)threadIdx.x; }
    __device__ int size() const { return (int)blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ bool all(bool p) const { return __syncthreads_and(p) != 0; }
    __device__ bool any(bool p) const { return __syncthreads_or(p) != 0; }
    __device__ int wave() const { return (int)(threadIdx.x >> 6); }
    __device__ int waves() const { return (int)(blockDim.x >> 6); }
    template <class F> __device__ void lanes(F f) const { f((int)(threadIdx.x & 63u)); }
    __device__ bool wave_all(bool p) const { return __builtin_amdgcn_ballot_w64(!p) == 0; }       // over the live lanes of the wavefront
    __device__ bool wave_leader() const { return (threadIdx.x & 63u) == 0; }
    // LDS operations of one wavefront execute in order; what has to be stopped is the compiler moving a lane's reads of OTHER
    // lanes' entries above its own writes (different addresses to it)
    __device__ void wave_sync() const
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __device__ void loads_issued() const { __builtin_amdgcn_sched_barrier(0); }
    __device__ uint32_t amb_load(const uint16_t* p) const
    {
        if (COHERENT) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return *p;
    }
    __device__ void amb_store(uint16_t* p, uint32_t v) const
    {
        if (COHERENT) __hip_atomic_store(p, (uint16_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *p = (uint16_t)v;
    }
};
using BlockDev = BlockDevT<false>;

// Tiles of the blur launches lie on an absolute 64 x 16 grid of the half-res map (so that the flags one launch leaves per tile
// mean the same tile to the next); a launch covers the tile rows that intersect its rows [row0, row1).
__device__ __forceinline__ BlurTileArgs blur_tile_args(const crychic_ssao_constants& cb, const EdgePlane& edge, const uint16_t* in, uint16_t* out,
                                                       uint32_t W, uint32_t H, uint32_t row0, uint32_t row1)
{
    // Natural order: consecutive tiles of a row go to different XCDs.  The blur's planes are small (they live in L2 / Infinity
    // Cache whatever the placement), but its cost is very uneven -- settled (sky, open ground) tiles cost nothing, the others sit
    // in the lower half of the frame -- and stripes of tile rows per XCD left one XCD with twice the work of the others.
    uint32_t bx = blockIdx.x, by = blockIdx.y;
    by += row0 / (uint32_t)kBlurTileH;
    BlurTileArgs a;
    a.w = &cb.BlurWeights[0][0];
    a.e = edge;
    a.in = in;
    a.out = out;
    a.w2 = (int)(W / 2);
    a.h2 = (int)(H / 2);
    a.x0 = (int)bx * kBlurTileW;
    a.y0 = (int)by * kBlurTileH;
    a.row0 = (int)row0;
    a.row1 = (int)row1;
    a.borderZ = ndc_to_view(cb, 1.0f);
    a.tileIndex = by * blur_tiles_x(W) + bx;
    return a;
}

// Iteration 0 of the blur: horizontal + vertical sweep of a tile in one launch (blur_tiles.hpp blur_pair_tile).
template <bool RECORD>
__global__ __launch_bounds__(512) void blur_pair_kernel(crychic_ssao_constants cb, EdgePlane edge, const uint16_t* __restrict__ in,
                                                        uint16_t* __restrict__ out, uint32_t W, uint32_t H, uint32_t row0, uint32_t row1,
                                                        uint32_t stamp, int onesMargin, int ssaoRow0, int ssaoRow1, uint32_t frameStamp)
{
    __shared__ f4a s_nz[kBlurPairSW * kBlurPairSH];
    __shared__ float s_a[kBlurPairSW * kBlurPairSH];
    __shared__ float s_mid[kBlurTileW * kBlurPairSH];
    __shared__ uint16_t s_hmask[kBlurTileW * kBlurTileH];
    const BlurTileArgs a = blur_tile_args(cb, edge, in, out, W, H, row0, row1);
    // The tile's counter of the single-launch chain that follows (blur_replay_chain_kernel): this frame's tag, no iteration done.
    // Written here, one launch earlier, so that every counter the chain polls was written in this frame -- whatever the workspace
    // held before, it cannot read as a neighbour's progress.
    if (RECORD && threadIdx.x == 0) edge.progress[a.tileIndex] = (unsigned long long)frameStamp << 8;
    blur_pair_tile<RECORD>(BlockDev{}, a, stamp, onesMargin, ssaoRow0, ssaoRow1, s_nz, s_a, s_mid, s_hmask);
}

// A later iteration of the blur, both sweeps, replayed (blur_tiles.hpp blur_replay_tile): 8 wavefronts per tile.
__global__ __launch_bounds__(512) void blur_replay_kernel(crychic_ssao_constants cb, EdgePlane edge, const uint16_t* __restrict__ in,
                                                          uint16_t* __restrict__ out, uint32_t W, uint32_t H, uint32_t row0, uint32_t row1,
                                                          uint32_t stamp, int onesShortcut)
{
    __shared__ float s_in[kBlurPairSW * kBlurPairSH];
    __shared__ uint32_t s_mask[kBlurPairSW * kBlurPairSH];
    __shared__ float s_mid[kBlurTileW * kBlurPairSH];
    __shared__ uint32_t s_rows[kBlurMaxWaves];
    const BlurTileArgs a = blur_tile_args(cb, edge, in, out, W, H, row0, row1);
    blur_replay_tile(BlockDev{}, a, stamp, onesShortcut != 0, s_in, s_mask, s_mid, s_rows);
}

// Iterations 1 .. blurCount - 1 of the chain in ONE launch: workgroup (x, y, z) replays iteration z + 1 of tiles (2 x, y) and
// (2 x + 1, y).  What the per-iteration launches get from the kernel boundary -- iteration j reads what iteration j - 1 wrote,
// and may overwrite the plane
// iteration j - 1 read -- is a per-tile dependency here: a tile's iteration j needs its own and its eight neighbours' iteration
// j - 1 COMPLETE (their outputs are its apron; their inputs are the plane it writes).  Every tile publishes its count of completed
// iterations, tagged with the frame stamp (a stale or uninitialised word never matches), after every wavefront of it has drained
// its write-through stores; a workgroup polls its tiles' predecessors (relaxed) and executes one agent-scope acquire before it
// stages (the hand-off's contract: DESIGN.md "Blur: one launch for the replayed iterations").  Forward progress: workgroups are dispatched in
// increasing (z, y, x) order and a workgroup only ever waits for workgroups of the layer below, which were dispatched before it
// and wait for nothing above them.  The poll is bounded all the same: a workgroup that gives up sets EdgePlane::progress's error
// word and goes on (wrong pixels, never a hang).  Tiles the pair launch settled neither work nor publish nor are waited for.
// Same bits as blur_replay_kernel: the tile body is blur_replay_tile's, split (blur_tiles.hpp blur_replay_fetch_masks / _rows /
// _cols).  What the launch buys is the launch boundaries: two of the chain's four drain-and-refill gaps, and a tile's iteration
// j + 1 can start while other tiles are still in iteration j.
// What the wait costs is the acquire, and it is paid per WORKGROUP that executes one on a CU.  So (CRY_BLUR_CHAIN_TILES = 2) a
// workgroup of 1024 threads replays TWO horizontally adjacent tiles -- wavefronts 0 .. 7 tile (2 bx, y), wavefronts 8 .. 15 tile
// (2 bx + 1, y), each half over LDS arrays of its own -- behind ONE poll set (the up to 12 counters of the 4 x 3 neighbourhood:
// the columns within one of a tile of the pair that works, settled and out-of-grid tiles skipped), ONE acquire and one barrier;
// after the common drain and barrier each tile's first lane publishes its counter.  A half whose tile is settled, lies outside
// the grid (odd tile count) or outside the iteration's rows skips the body and meets every barrier all the same (the barriers
// are in this kernel's uniform control flow, none inside the halves of the body); a workgroup both of whose tiles are settled
// returns at once.  And every lane fetches its six recorded decision words (written by the pair launch, by no workgroup of this
// one) BEFORE the poll: they travel while wavefront 0 waits for the neighbours and for the invalidate.
// Forward progress, restated for pairs: the grid is (ceil(tiles_x / 2), y, z), dispatched in increasing (z, y, x) order as
// before; a workgroup of layer z waits only for counters of tiles of layer z - 1, each published by a workgroup of layer z - 1,
// all of which were dispatched before it and wait for nothing of layer z or above.
#ifndef CRY_BLUR_CHAIN_TILES
#define CRY_BLUR_CHAIN_TILES 2        // tiles per workgroup of blur_replay_chain_kernel (1: the probe build's one tile per workgroup)
#endif
#ifndef CRY_BLUR_CHAIN_SLEEP
#define CRY_BLUR_CHAIN_SLEEP 16       // s_sleep between two polls of a counter (units of 64 clocks)
#endif
struct BlurChainPlan {
    uint16_t* plane[2];
    uint32_t row0[8], row1[8];      // half-res rows of its output iteration z + 1 owes
    uint32_t in[8];                 // plane index it reads (writes the other)
    uint32_t tileRow0;              // first tile row of the grid (absolute 64 x 16 grid)
};
// The eight wavefronts of ONE tile inside a workgroup of TILES tiles, as the split tile body sees them.
struct BlockChainTile : BlockDevT<true> {
    __device__ int wave() const { return (int)((threadIdx.x >> 6) & (uint32_t)(kBlurMaxWaves - 1)); }
    __device__ int waves() const { return kBlurMaxWaves; }
};
template <int TILES>
__global__ __launch_bounds__(512 * TILES) void blur_replay_chain_kernel(crychic_ssao_constants cb, EdgePlane edge, BlurChainPlan plan, uint32_t W,
                                                                        uint32_t H, uint32_t stamp, uint32_t exitStamp, int onesShortcut)
{
    static_assert(TILES == 1 || TILES == 2, "one tile or a pair per workgroup");
    constexpr int NW = kBlurMaxWaves, NC = TILES + 2;          // wavefronts per tile; tile columns of the neighbourhood
    __shared__ float s_in[TILES][kBlurPairSW * kBlurPairSH];
    __shared__ float s_mid[TILES][kBlurTileW * kBlurPairSH];
    __shared__ uint32_t s_rows[TILES][kBlurMaxWaves];
    const uint32_t half = TILES == 2 ? threadIdx.x >> 9 : 0u;
    const uint32_t it = blockIdx.z, tx0 = blockIdx.x * (uint32_t)TILES, ty = plan.tileRow0 + blockIdx.y, ntx = blur_tiles_x(W);
    // live: in the grid and not settled (settled: 65535 in both planes, for good)
    bool live[2] = { false, false };
#pragma unroll
    for (int t = 0; t < TILES; ++t) live[t] = tx0 + (uint32_t)t < ntx && !(exitStamp != 0u && edge.tiles[ty * ntx + tx0 + (uint32_t)t] == exitStamp);
    if (!live[0] && !live[1]) return;
    const uint32_t tx = tx0 + half, tile = ty * ntx + tx;
    const bool liveHere = half ? live[1] : live[0];
    const uint32_t row0 = plan.row0[it], row1 = plan.row1[it];
    const bool mine = ty * (uint32_t)kBlurTileH < row1 && (ty + 1u) * (uint32_t)kBlurTileH > row0;
    const bool work = liveHere && mine;
    BlurTileArgs a;
    a.w = &cb.BlurWeights[0][0];
    a.e = edge;
    a.in = plan.plane[plan.in[it]];
    a.out = plan.plane[plan.in[it] ^ 1u];
    a.w2 = (int)(W / 2);
    a.h2 = (int)(H / 2);
    a.x0 = (int)tx * kBlurTileW;
    a.y0 = (int)ty * kBlurTileH;
    a.row0 = (int)row0;
    a.row1 = (int)row1;
    a.borderZ = ndc_to_view(cb, 1.0f);
    a.tileIndex = tile;
    const BlockChainTile blk{};
    BlurReplayMasks<BlockChainTile, NW> mk;
    if (work) blur_replay_fetch_masks<NW>(blk, a, mk);            // issued here, used behind the barrier
    const unsigned long long tag = (unsigned long long)stamp << 8;
    if (it > 0u) {
        // wait for the neighbourhood's iteration `it` (count >= it), lanes 0 .. 3 NC - 1 of the first wavefront one tile each
        if (threadIdx.x < (uint32_t)(3 * NC)) {
            const int off = (int)(threadIdx.x % (uint32_t)NC) - 1;               // tile column relative to the pair's left tile
            const int nx = (int)tx0 + off, ny = (int)ty + (int)(threadIdx.x / (uint32_t)NC) - 1;
            const bool wanted = (live[0] && off <= 1) || (live[1] && off >= 0);      // within one column of a tile that is not settled
            const bool inGrid = wanted && nx >= 0 && nx < (int)ntx && ny >= (int)plan.tileRow0 && ny < (int)(plan.tileRow0 + gridDim.y);
            if (inGrid) {
                const uint32_t n = (uint32_t)ny * ntx + (uint32_t)nx;
                if (!(exitStamp != 0u && edge.tiles[n] == exitStamp)) {
                    bool ok = false;
                    for (int spin = 0; spin < (1 << 16) && !ok; ++spin) {
                        // relaxed polls (global_load_dwordx2 sc1: a coherent load, no cache invalidation per poll -- an acquire here
                        // flushed the caches under the workgroups that were doing the work, 14x slower); the ONE acquire of the
                        // hand-off follows the wait, below
                        const unsigned long long v = __hip_atomic_load(edge.progress + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ok = (v >> 8) == (tag >> 8) && (v & 255ull) >= (unsigned long long)it;
                        if (!ok) __builtin_amdgcn_s_sleep(CRY_BLUR_CHAIN_SLEEP);
                    }
                    if (!ok) edge.progress[(size_t)ntx * blur_tiles_y(H)] = tag | 255ull;      // the error word (one past the tiles)
                }
            }
            // Consumer side of the hand-off, the acquire kept rather than one of the acquire-free forms measured safe (those need
            // 4-byte or wider texels, or whole 128-byte lines per store instruction, which 2-byte texels on ragged widths are
            // not): the polling wavefront, once every poll of it has matched, executes ONE agent-scope acquire (s_waitcnt
            // vmcnt(0); buffer_inv sc1: this CU's L1 only) and waits for it (s_waitcnt vmcnt(0)) before it joins the barrier that
            // lets the other wavefronts load.  Inside this branch, so that every path from the poll passes it.  The staging
            // loads stay device-coherent (sc1) as well.
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
    }
    if (work) blur_replay_rows<NW>(blk, a, onesShortcut != 0, mk, s_in[half], s_mid[half], s_rows[half]);
    __syncthreads();
    if (work) blur_replay_cols<NW>(blk, a, mk, s_mid[half], s_rows[half]);
    // Producer side.  The tile's outputs were device-coherent (write-through, sc1) stores: once EVERY wavefront has seen its own
    // stores acknowledged (s_waitcnt vmcnt(0), written as inline assembly: a workgroup-scope release fence emits no vmcnt wait
    // here, and s_barrier waits for no counter) and has then reached the barrier, the texels are visible to every XCD and one
    // lane may publish the count (a relaxed agent-scope store: global_store_dwordx2 sc1) -- no L2 write-back (an agent-scope
    // release fence per workgroup writes back the XCD's whole L2: measured 390 us for the launch).
    // tools/handoff_isa.py checks this order in the emitted assembly on every path (tests/test_chain_handoff_isa.py).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if ((threadIdx.x & 511u) == 0 && liveHere)
        __hip_atomic_store(edge.progress + tile, tag | (unsigned long long)(it + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool ZERO_RADIUS, bool FIX, bool MIPS = false>
__global__ __launch_bounds__(256) void light_kernel(LightParams P, const f4a* __restrict__ g0,
                                                    const f4a* __restrict__ g1, const f4a* __restrict__ g2,
                                                    const uint32_t* __restrict__ depth,
                                                    const uint16_t* __restrict__ ambient,
                                                    const uint32_t* __restrict__ cube, uint32_t* __restrict__ out,
                                                    f4a* __restrict__ radiance, uint32_t row0, uint32_t row1)
{
    light_frame_tile<ZERO_RADIUS, FIX, CubeOfMips<MIPS>>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1);
}

template <bool ZERO_RADIUS, bool MIPS = false>
__global__ __launch_bounds__(256) void light_points_kernel(LightParams P, const f4a* __restrict__ g0, const f4a* __restrict__ g1,
                                                           const f4a* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                           const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                           uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                           uint32_t row1)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    light_local_tile<ZERO_RADIUS, CubeOfMips<MIPS>, false>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1, s_box, s_mask, nullptr, 0u, nullptr);
}

// The same pass with `numSpots` (1 .. 1024) spot lights after the point lights (crychic_deferred_light_spots); zero spot lights
// take light_points_kernel / light_kernel, so this kernel is never the reference configuration's.
template <bool ZERO_RADIUS, bool MIPS = false>
__global__ __launch_bounds__(256) void light_spots_kernel(LightParams P, const f4a* __restrict__ g0, const f4a* __restrict__ g1,
                                                          const f4a* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                          const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                          uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                          uint32_t row1, const crychic_light* __restrict__ spots, uint32_t numSpots)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    __shared__ uint32_t s_spotMask[kMaxSpotLights / 32];
    light_local_tile<ZERO_RADIUS, CubeOfMips<MIPS>, true>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1, s_box, s_mask, spots, numSpots, s_spotMask);
}

// The same pass with the first shadows.count (1 .. 8) spot lights shadowed (crychic_deferred_light_spots_shadowed); a count of 0
// takes light_spots_kernel, so none of the instantiations above changes.
template <bool ZERO_RADIUS, bool MIPS>
__global__ __launch_bounds__(256) void light_spots_shadowed_kernel(LightParams P, const f4a* __restrict__ g0, const f4a* __restrict__ g1,
                                                                   const f4a* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                                   const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                                   uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                                   uint32_t row1, const crychic_light* __restrict__ spots, uint32_t numSpots,
                                                                   SpotShadows shadows)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    __shared__ uint32_t s_spotMask[kMaxSpotLights / 32];
    light_local_tile<ZERO_RADIUS, CubeOfMips<MIPS>, true, true>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1, s_box, s_mask,
                                                                spots, numSpots, s_spotMask, &shadows);
}

// The same pass with the first pointShadows.count (1 .. 4) point lights shadowed (crychic_deferred_light_point_shadows), spot lights
// and their shadows as light_spots_shadowed_kernel: zero spot lights or a spot shadow count of 0 are settled at run time (SpotShadowOf
// returns 1, the unshadowed bits).  A point shadow count of 0 takes the kernels above, so none of their instantiations changes.
template <bool ZERO_RADIUS, bool MIPS>
__global__ __launch_bounds__(256) void light_point_shadows_kernel(LightParams P, const f4a* __restrict__ g0, const f4a* __restrict__ g1,
                                                                  const f4a* __restrict__ g2, const uint32_t* __restrict__ depth,
                                                                  const uint16_t* __restrict__ ambient, const uint32_t* __restrict__ cube,
                                                                  uint32_t* __restrict__ out, f4a* __restrict__ radiance, uint32_t row0,
                                                                  uint32_t row1, const crychic_light* __restrict__ spots, uint32_t numSpots,
                                                                  SpotShadows shadows, PointShadows pointShadows)
{
    __shared__ float s_box[4][6];
    __shared__ uint32_t s_mask[kMaxPointLights / 32];
    __shared__ uint32_t s_spotMask[kMaxSpotLights / 32];
    light_local_tile<ZERO_RADIUS, CubeOfMips<MIPS>, true, true, true>(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, row1, s_box,
                                                                      s_mask, spots, numSpots, s_spotMask, &shadows, &pointShadows);
}
// Its kernel arguments, the largest of any kernel here: the usual HIP limit is 4 KiB.
static_assert(sizeof(LightParams) + sizeof(SpotShadows) + sizeof(PointShadows) + 9 * sizeof(void*) + 3 * sizeof(uint32_t) <= 4096,
              "light_point_shadows_kernel's arguments exceed 4 KiB");

// ---- launchers ---------------------------------------------------------------------------------------------------
// Margin (depth texel rows) of a row-limited depth pass around the rows of the call (ssao_core.hpp depth_pass_cell_rows).  Any value
// gives the same pixels (tests: margins 0, 8, 40 with everything unvisited poisoned); CRYCHIC_DEPTH_MARGIN is the tuning knob the
// strips rehearsal sweeps (tools/strips_rehearsal.sh), unset = the default rule (H / 11, at least 64).
static int depth_margin()
{
    static const int m = [] { const char* e = getenv("CRYCHIC_DEPTH_MARGIN"); return e ? atoi(e) : -1; }();
    return m;
}

hipError_t launch_depth_pairs(const crychic_ssao_constants& cb, const uint32_t* depth, void* edge_base, uint32_t W, uint32_t H, uint32_t stamp,
                              bool writePairs, uint32_t row0, uint32_t rows, hipStream_t stream)
{
    const EdgePlane e = edge_plane_carve(edge_base, W, H);
    uint32_t c0, cn;
    depth_pass_cell_rows(H, row0, rows, &c0, &cn, depth_margin());
    if (cn == 0) return hipSuccess;
    // a wavefront per 128 entry columns x 8 entry rows (= one row of 16 cells of the nearest-depth map), four wavefronts per workgroup
    const uint32_t segs = (depth_pairs_pitch(W) / 2u + 63u) / 64u;
    const dim3 grid((segs + 3u) / 4u, cn, 1);
#define CRY_LAUNCH_DP(K) hipLaunchKernelGGL(K, grid, dim3(256), 0, stream, depth, (f4a*)const_cast<void*>(e.pairs), e.geo, e.zcull, stamp, W, H, \
                                            ssao_cull_params(cb), c0)
    if (writePairs) CRY_LAUNCH_DP(depth_pairs_kernel<true>); else CRY_LAUNCH_DP(depth_pairs_kernel<false>);
#undef CRY_LAUNCH_DP
    return hipGetLastError();
}

hipError_t launch_ssao(const crychic_ssao_constants& cb, const void* normal, const uint32_t* depth,
                       const uint8_t* randvec, uint16_t* ambient, void* edge_base, uint32_t W, uint32_t H,
                       uint32_t row0, uint32_t rows, bool emit_ao, bool use_pairs, uint32_t stamp, hipStream_t stream)
{
    if (rows == 0) return hipSuccess;
    EdgePlane e{};
    if (edge_base) e = edge_plane_carve(edge_base, W, H);
    if (use_pairs && !edge_base) return hipErrorInvalidValue;
    dim3 grid = grid_for(W / 2, rows);
    // super-tiles of SX x SY workgroup tiles (64 x 4 half-res pixels each) per XCD; the grid is padded to whole super-tiles.
    // 2 x 16 tiles = 128 x 64 half-res pixels.  Round 2 ran 4 x 32 (every tap gathered: L2 locality of the gathers decided); with
    // the tap culling only one tap in seven gathers and the balance between XCDs -- sky is cheap, near ground is not -- weighs
    // more: 4K 81.7 -> 77.4 us for the pass, 1080p 33.4 -> 31.7, covered camera equal, 8K +1.5 % (natural order: 77.5 / 31.4 /
    // +2 % / +3 %; profiles/r03_supertile_sweep.txt)
    uint32_t SX = 2u, SY = 16u;
    SX = SX > grid.x ? grid.x : SX;
    SY = SY > grid.y ? grid.y : SY;
    grid.x = (grid.x + SX - 1u) / SX * SX;
    grid.y = (grid.y + SY - 1u) / SY * SY;
    const int sparse = ssao_projtex_is_sparse(cb) ? 1 : 0;
    SkyReach sky = ssao_sky_reach(cb, W, H);
    const bool maps = edge_base && stamp != 0u;        // stamp 0: the caller did not run the depth pass
    if (!maps) sky.enabled = 0;
    const int cull = (maps && ssao_cull_params(cb).enabled) ? 1 : 0;
    // what launch_depth_pairs prepared for these rows: everything, or footprint rows j0 with 8 c0 <= j0 + 2 < 8 (c0 + cn)
    uint32_t c0, cn;
    depth_pass_cell_rows(H, row0, rows, &c0, &cn, depth_margin());
    const bool limitedRows = maps && (c0 > 0u || c0 + cn < zmin_map_rows(H));
    const bool limited = limitedRows && use_pairs;
    const PrepRows prep{ 8 * (int)c0 - 2, 8u * cn };
    if (limitedRows) {                  // geometry-map cells are known for the texel rows the pass visited (8 entry rows per cell row)
        sky.y0 = 8 * (int)c0 - 2 < 0 ? 0 : 8 * (int)c0 - 2;
        sky.y1 = 8 * (int)(c0 + cn) - 2 > (int)H ? (int)H : 8 * (int)(c0 + cn) - 2;
    }
#define CRY_LAUNCH_SSAO(K) hipLaunchKernelGGL(K, grid, dim3(256), 0, stream, cb, (const u2*)normal, depth, (const uint32_t*)randvec, ambient, e, W, H, row0, row0 + rows, SX, SY, sparse, sky, stamp, cull, prep, half_res_scale(W, H))
    if (!emit_ao) CRY_LAUNCH_SSAO((ssao_kernel<false, false, false, false>));
    else if (limited) CRY_LAUNCH_SSAO((ssao_kernel<true, true, true, true>));
    else if (limitedRows) CRY_LAUNCH_SSAO((ssao_kernel<true, false, true, true>));
    else if (use_pairs && maps) CRY_LAUNCH_SSAO((ssao_kernel<true, true, true, false>));
    else if (use_pairs) CRY_LAUNCH_SSAO((ssao_kernel<true, true, false, false>));
    else if (maps) CRY_LAUNCH_SSAO((ssao_kernel<true, false, true, false>));
    else CRY_LAUNCH_SSAO((ssao_kernel<true, false, false, false>));
#undef CRY_LAUNCH_SSAO
    return hipGetLastError();
}

hipError_t launch_blur(const crychic_ssao_constants& cb, const void* edge_base, const uint16_t* in, uint16_t* out,
                       uint32_t W, uint32_t H, bool horizontal, uint32_t row0, uint32_t rows, hipStream_t stream)
{
    if (rows == 0) return hipSuccess;
    const EdgePlane e = edge_plane_carve(const_cast<void*>(edge_base), W, H);
    const dim3 grid = grid_for(W / 2, rows, 16u);
    if (horizontal) hipLaunchKernelGGL(blur_kernel<true>, grid, dim3(256), 0, stream, cb, e, in, out, W, H, row0, row0 + rows);
    else hipLaunchKernelGGL(blur_kernel<false>, grid, dim3(256), 0, stream, cb, e, in, out, W, H, row0, row0 + rows);
    return hipGetLastError();
}

// tile rows of the absolute 64 x 16 grid that intersect half-res rows [row0, row0 + rows)
static inline dim3 blur_tile_grid(uint32_t W, uint32_t row0, uint32_t rows)
{
    const uint32_t t0 = row0 / (uint32_t)kBlurTileH, t1 = (row0 + rows - 1u) / (uint32_t)kBlurTileH;
    return dim3(blur_tiles_x(W), t1 - t0 + 1u, 1);
}

hipError_t launch_blur_pair(const crychic_ssao_constants& cb, const void* edge_base, const uint16_t* in, uint16_t* out, uint32_t W, uint32_t H,
                            uint32_t row0, uint32_t rows, bool record, uint32_t stamp, int onesMargin, uint32_t ssaoRow0, uint32_t ssaoRows,
                            hipStream_t stream)
{
    if (rows == 0) return hipSuccess;
    const EdgePlane e = edge_plane_carve(const_cast<void*>(edge_base), W, H);
    // the unoccluded-tile exit needs finite positive weights (x * rcp(x) of a finite positive total) and the SSAO pass's map
    const uint32_t frameStamp = stamp;
    if (!blur_weights_positive(cb)) stamp = 0u;
    const dim3 grid = blur_tile_grid(W, row0, rows);
#define CRY_LAUNCH_PAIR(K) hipLaunchKernelGGL(K, grid, dim3(512), 0, stream, cb, e, in, out, W, H, row0, row0 + rows, stamp, onesMargin, \
                                              (int)ssaoRow0, (int)(ssaoRow0 + ssaoRows), frameStamp)
    if (record) CRY_LAUNCH_PAIR(blur_pair_kernel<true>); else CRY_LAUNCH_PAIR(blur_pair_kernel<false>);
#undef CRY_LAUNCH_PAIR
    return hipGetLastError();
}

hipError_t launch_blur_replay(const crychic_ssao_constants& cb, const void* edge_base, const uint16_t* in, uint16_t* out, uint32_t W, uint32_t H,
                              uint32_t row0, uint32_t rows, uint32_t stamp, hipStream_t stream)
{
    if (rows == 0) return hipSuccess;
    const EdgePlane e = edge_plane_carve(const_cast<void*>(edge_base), W, H);
    const int ones = blur_weights_positive(cb) ? 1 : 0;
    if (!ones) stamp = 0u;             // the pair launch settled no tile either
    hipLaunchKernelGGL(blur_replay_kernel, blur_tile_grid(W, row0, rows), dim3(512), 0, stream, cb, e, in, out, W, H, row0, row0 + rows, stamp, ones);
    return hipGetLastError();
}

hipError_t launch_blur_replay_chain(const crychic_ssao_constants& cb, const void* edge_base, uint16_t* plane0, uint16_t* plane1, uint32_t W, uint32_t H,
                                    int blurCount, uint32_t row0, uint32_t rows, uint32_t stamp, hipStream_t stream)
{
    const int n = blurCount - 1;                       // replay iterations 1 .. blurCount - 1
    if (n <= 0 || rows == 0) return hipSuccess;
    if (n > 8) return hipErrorInvalidValue;
    const EdgePlane e = edge_plane_carve(const_cast<void*>(edge_base), W, H);
    BlurChainPlan plan;
    plan.plane[0] = plane0;
    plan.plane[1] = plane1;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (int i = 1; i <= n; ++i) {
        const BlurStep st = blur_chain_step(blurCount, row0, rows, H / 2u, i);
        plan.row0[i - 1] = st.row0;
        plan.row1[i - 1] = st.row0 + st.rows;
        plan.in[i - 1] = (uint32_t)st.in;
        if (st.rows) { lo = st.row0 < lo ? st.row0 : lo; hi = st.row0 + st.rows > hi ? st.row0 + st.rows : hi; }
    }
    for (int i = n; i < 8; ++i) { plan.row0[i] = plan.row1[i] = 0u; plan.in[i] = 0u; }
    if (hi <= lo) return hipSuccess;
    const dim3 g = blur_tile_grid(W, lo, hi - lo);
    plan.tileRow0 = lo / (uint32_t)kBlurTileH;
    const int ones = blur_weights_positive(cb) ? 1 : 0;
    constexpr unsigned T = CRY_BLUR_CHAIN_TILES;       // tiles of a row per workgroup
    hipLaunchKernelGGL(blur_replay_chain_kernel<(int)T>, dim3((g.x + T - 1u) / T, g.y, (unsigned)n), dim3(512u * T), 0, stream, cb, e, plan, W, H, stamp,
                       ones ? stamp : 0u, ones);
    return hipGetLastError();
}

hipError_t launch_light(const LightParams& P, const float* g0, const float* g1, const float* g2,
                        const uint32_t* depth, const uint16_t* ambient, const uint8_t* cube, uint8_t* out,
                        float* radiance, uint32_t row0, uint32_t rows, hipStream_t stream, const crychic_light* spots,
                        uint32_t numSpots, const SpotShadows* shadows, const PointShadows* pointShadows)
{
    if (rows == 0) return hipSuccess;
    const dim3 grid = grid_for(P.W, rows);
    // the derivative chain: quads inside wavefronts (light_tile_pixel), so the rows must start a quad
    const bool mips = light_variant(P.flags, P.cubeLevels).lookup == CubeLookup::DerivativeChain;
    if (mips && (row0 & 1u)) return hipErrorInvalidValue;
    // every family shares the kernel arguments up to row1; launch(kernel, extra...) appends the family's own
    auto launch = [&](auto kernel, auto... extra) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, P, (const f4a*)g0, (const f4a*)g1, (const f4a*)g2, depth, ambient,
                           (const uint32_t*)cube, (uint32_t*)out, (f4a*)radiance, row0, row0 + rows, extra...);
    };
    // by_radius(f) calls f(z) once and dispatch(family) calls family(z, m) once: z = <ZERO_RADIUS>, m = <MIPS>, as std::bool_constant
    auto by_radius = [&](auto f) {
        if (P.pcfSearchRadius == 0.0f) f(std::true_type{}); else f(std::false_type{});
        return hipGetLastError();
    };
    auto dispatch = [&](auto family) {
        return by_radius([&](auto z) { if (mips) family(z, std::true_type{}); else family(z, std::false_type{}); });
    };
    const LightFamily family = light_family(P.flags, P.numPointLights, numSpots, shadows ? shadows->count : 0u,
                                            pointShadows ? pointShadows->count : 0u, P.cubeLevels);
    switch (family) {
    case LightFamily::FormatsFrame:
    case LightFamily::FormatsLocal:               // a half4 plane or a flagged lookup, ambient or specular term (light_general.hip)
        return launch_light_general(P, g0, g1, g2, depth, ambient, cube, out, radiance, row0, rows, stream, spots, numSpots, shadows, pointShadows);
    case LightFamily::PointShadows:
        return dispatch([&](auto z, auto m) { launch(light_point_shadows_kernel<z, m>, spots, numSpots, shadows ? *shadows : SpotShadows{},
                                                     *pointShadows); });
    case LightFamily::SpotsShadowed:
        return dispatch([&](auto z, auto m) { launch(light_spots_shadowed_kernel<z, m>, spots, numSpots, *shadows); });
    case LightFamily::Spots:
        return dispatch([&](auto z, auto m) { launch(light_spots_kernel<z, m>, spots, numSpots); });
    case LightFamily::Points:
        return dispatch([&](auto z, auto m) { launch(light_points_kernel<z, m>); });
    case LightFamily::FrameFix:
    case LightFamily::Frame:
        if (mips)                                 // FrameFix: FIX compiled in, the chain is not the benchmark's instantiation
            return by_radius([&](auto z) { launch(light_kernel<z, true, true>); });
        return by_radius([&](auto z) { if (family == LightFamily::FrameFix) launch(light_kernel<z, true>); else launch(light_kernel<z, false>); });
    }
    return hipErrorInvalidValue;
}

}  // namespace cry
