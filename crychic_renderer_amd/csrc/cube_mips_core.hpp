// cube_mips_core.hpp -- the per-tile body of crychic_generate_cube_mips (cube_mips.hip), written so that a
// host compiler builds it too (tests/cube_mips_host): one call per thread and phase, the caller supplies the barrier between phases.
//
// Definition (include/crychic_hip.h): level k+1, face f, texel (x, y), channel c = (a + b + c' + d + 2) >> 2 over the level-k texels
// (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1) of the same face -- geometry.box_mips, byte for byte.  Texel x of level k+1 reads
// texels 2x and 2x+1 of level k, so a 64-aligned tile of a level owns its whole pyramid down to one texel: a workgroup of 256
// threads reduces one 64 x 64 tile of one face of the launch's input level through up to six levels and never meets another
// workgroup; ragged and odd sizes are masks on the output coordinates (the last row and column of an odd level are never read,
// because 2x+1 <= 2 (d >> 1) - 1 < d for every output x < d >> 1).
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

constexpr uint32_t kCubeMipTile = 64u;           // texels per side of a tile of the launch's input level
constexpr uint32_t kCubeMipTileLevels = 6u;      // levels a tile yields: 32, 16, 8, 4, 2, 1 texels per side
constexpr uint32_t kCubeMipThreads = 256u;
// The tile's pyramid in LDS, one region per level so that a level is never read and written in the same phase:
// level j (1 .. 6) holds (64 >> j)^2 words at cube_mip_tile_offset(j).
constexpr uint32_t kCubeMipTileWords = 1024u + 256u + 64u + 16u + 4u + 1u;
CRY_HD uint32_t cube_mip_tile_offset(uint32_t j) { return (4096u - (4096u >> (2u * (j - 1u)))) / 3u; }     // 0, 1024, 1280, 1344, 1360, 1364

CRY_HD uint32_t cube_mip_dim(uint32_t dim, uint32_t level) { return (level < 32u && (dim >> level)) ? (dim >> level) : 1u; }
CRY_HD size_t cube_level_texels(uint32_t d) { return (size_t)6u * d * d; }
// floor(log2 dim) + 1: the levels of a chain that ends at 1 x 1
CRY_HD uint32_t cube_full_levels(uint32_t dim) { uint32_t n = 1u; for (uint32_t m = dim; m > 1u; m >>= 1) ++n; return n; }

// Four RGBA8 texels -> their rounded mean, channel by channel.  The channels are widened to 16-bit integers two at a time (R and B
// in one word, G and A in the other): a sum of four bytes plus 2 is at most 1022 and never carries into its neighbour.
CRY_HD uint32_t cube_mip_mean4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t m = 0x00FF00FFu;
    const uint32_t rb = (a & m) + (b & m) + (c & m) + (d & m) + 0x00020002u;
    const uint32_t ga = ((a >> 8) & m) + ((b >> 8) & m) + ((c >> 8) & m) + ((d >> 8) & m) + 0x00020002u;
    return ((rb >> 2) & m) | (((ga >> 2) & m) << 8);
}

// Native 16-byte and 8-byte vectors for the aligned loads (four texels) and stores (two texels): one memory instruction each.
typedef uint32_t CubeMipTexels4 __attribute__((ext_vector_type(4)));
typedef uint32_t CubeMipTexels2 __attribute__((ext_vector_type(2)));

// Phase 1, thread t of 256: level `in` (dIn x dIn texels, face base `src`) -> the next level (dOut = dIn >> 1, face base `dst`) and
// region 1 of `tile`.  A thread owns a column of four input texels (two output texels) in row pairs t / 16 and t / 16 + 16 of the
// tile: its 2 x 2 sums are its own.  VEC: dIn is a multiple of 4 and the chain 16-byte aligned -- 16-byte loads, 8-byte stores;
// otherwise dword accesses.  A template parameter, so that the two paths are two kernels and the compiler cannot
// merge a dword of one into the other (as an argument it split every 16-byte load into 12 + 4 bytes).
template <bool VEC>
CRY_HD void cube_mips_tile_first(const uint32_t* src, uint32_t* dst, uint32_t dIn, uint32_t tileX, uint32_t tileY, uint32_t t,
                                 uint32_t* tile)
{
    const uint32_t dOut = dIn >> 1;
    const uint32_t cx = t & 15u, ry = t >> 4;
    const uint32_t x = tileX * kCubeMipTile + 4u * cx;              // input column of the thread's first texel
    // Texels outside the level are never part of a stored mean (header comment), so a thread outside it reads the nearest texels
    // inside instead of branching: the four loads of a thread are issued back to back.
    CubeMipTexels4 r[2][2];                                          // [pass][row of the pair]
    size_t row[2][2];
    for (uint32_t p = 0; p < 2u; ++p)
        for (uint32_t q = 0; q < 2u; ++q) {
            const uint32_t y = tileY * kCubeMipTile + 2u * (ry + 16u * p) + q;
            row[p][q] = (size_t)(y < dIn ? y : dIn - 1u) * dIn;
        }
    for (uint32_t p = 0; p < 2u; ++p)
        for (uint32_t q = 0; q < 2u; ++q) {
            if (VEC) r[p][q] = *reinterpret_cast<const CubeMipTexels4*>(src + row[p][q] + (x < dIn ? x : dIn - 4u));
            else for (uint32_t i = 0; i < 4u; ++i) r[p][q][i] = src[row[p][q] + (x + i < dIn ? x + i : dIn - 1u)];
        }
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);          // all of a thread's loads before any of the arithmetic that waits for them
#endif
    for (uint32_t p = 0; p < 2u; ++p) {
        const uint32_t rp = ry + 16u * p;
        CubeMipTexels2 o;
        o[0] = cube_mip_mean4(r[p][0][0], r[p][0][1], r[p][1][0], r[p][1][1]);
        o[1] = cube_mip_mean4(r[p][0][2], r[p][0][3], r[p][1][2], r[p][1][3]);
        tile[rp * 32u + 2u * cx] = o[0];
        tile[rp * 32u + 2u * cx + 1u] = o[1];
        const uint32_t ox = tileX * 32u + 2u * cx, oy = tileY * 32u + rp;
        const size_t at = (size_t)oy * dOut + ox;
        if (oy < dOut) {
            if (VEC) {                                               // dOut is even: both texels or neither
                if (ox < dOut) *reinterpret_cast<CubeMipTexels2*>(dst + at) = o;
            } else {
                if (ox < dOut) dst[at] = o[0];
                if (ox + 1u < dOut) dst[at + 1u] = o[1];
            }
        }
    }
}

// Phase j (2 .. 6), thread t: region j - 1 of `tile` -> region j and level j of the launch (d x d texels, face base `dst`); the
// first (64 >> j)^2 threads each own one output texel.  The caller puts a barrier between two phases.
CRY_HD void cube_mips_tile_next(uint32_t* dst, uint32_t d, uint32_t j, uint32_t tileX, uint32_t tileY, uint32_t t, uint32_t* tile)
{
    const uint32_t s = kCubeMipTile >> j;
    if (t >= s * s) return;
    const uint32_t x = t & (s - 1u), y = t / s;
    const uint32_t* in = tile + cube_mip_tile_offset(j - 1u) + (2u * y) * (2u * s) + 2u * x;
    const uint32_t v = cube_mip_mean4(in[0], in[1], in[2u * s], in[2u * s + 1u]);
    tile[cube_mip_tile_offset(j) + y * s + x] = v;
    const uint32_t ox = tileX * s + x, oy = tileY * s + y;
    if (ox < d && oy < d) dst[(size_t)oy * d + ox] = v;
}

// The phases of one tile of one face, as thread t runs them: the level and offset walking of a launch.  levelIn: the first texel
// of the launch's input level (all six faces); the levels it yields follow it in memory, each six faces.
template <bool VEC>
CRY_HD void cube_mips_tile_phase_first(uint32_t* levelIn, uint32_t dIn, uint32_t face, uint32_t tileX, uint32_t tileY, uint32_t t,
                                       uint32_t* tile)
{
    const uint32_t d = dIn >> 1;
    uint32_t* out = levelIn + cube_level_texels(dIn);
    cube_mips_tile_first<VEC>(levelIn + (size_t)face * dIn * dIn, out + (size_t)face * d * d, dIn, tileX, tileY, t, tile);
}
CRY_HD void cube_mips_tile_phase_next(uint32_t* levelIn, uint32_t dIn, uint32_t j, uint32_t face, uint32_t tileX, uint32_t tileY,
                                      uint32_t t, uint32_t* tile)       // j = 2 .. 6
{
    uint32_t d = dIn >> 1;
    uint32_t* out = levelIn + cube_level_texels(dIn);
    for (uint32_t i = 2u; i <= j; ++i) {
        out += cube_level_texels(d);
        d >>= 1;
    }
    cube_mips_tile_next(out + (size_t)face * d * d, d, j, tileX, tileY, t, tile);
}

// One tile of one face through `nLevels` (1 .. 6) levels, as one thread runs it; `barrier` separates the phases.
template <bool VEC, typename Barrier>
CRY_HD void cube_mips_tile(uint32_t* levelIn, uint32_t dIn, uint32_t nLevels, uint32_t face, uint32_t tileX, uint32_t tileY, uint32_t t,
                           uint32_t* tile, Barrier barrier)
{
    cube_mips_tile_phase_first<VEC>(levelIn, dIn, face, tileX, tileY, t, tile);
    for (uint32_t j = 2u; j <= nLevels; ++j) {
        barrier();
        cube_mips_tile_phase_next(levelIn, dIn, j, face, tileX, tileY, t, tile);
    }
}

// The launch plan (cube_mips.hip's launcher and the host harness walk it): launch i takes level 6 i as its input and yields the
// next n = min(6, levels - 1 - 6 i) levels.  vec: the 16-byte path's condition for that launch.
struct CubeMipLaunch { uint32_t* levelIn; uint32_t dIn, nLevels, tiles; bool vec; };
CRY_HD uint32_t cube_mips_launches(uint32_t levels) { return (levels - 1u + kCubeMipTileLevels - 1u) / kCubeMipTileLevels; }
CRY_HD CubeMipLaunch cube_mips_launch(uint8_t* chain, uint32_t dim, uint32_t levels, uint32_t i)
{
    const uint32_t k = i * kCubeMipTileLevels;
    uint32_t* level = reinterpret_cast<uint32_t*>(chain);
    for (uint32_t j = 0; j < k; ++j) level += cube_level_texels(cube_mip_dim(dim, j));
    CubeMipLaunch L;
    L.levelIn = level;
    L.dIn = cube_mip_dim(dim, k);
    L.nLevels = levels - 1u - k < kCubeMipTileLevels ? levels - 1u - k : kCubeMipTileLevels;
    L.tiles = (L.dIn + kCubeMipTile - 1u) / kCubeMipTile;
    L.vec = L.dIn % 4u == 0u && (reinterpret_cast<uintptr_t>(level) & 15u) == 0u;
    return L;
}

}  // namespace cry
