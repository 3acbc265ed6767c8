// decal.hip -- crychic_apply_decals: deferred decals, box-projected textures blended into the G-buffer planes between the producer
// passes and the lighting pass.  One lane per pixel, an 8 x 8 pixel tile per wavefront, four tiles side by side
// per workgroup; a 1-D grid of tilesX workgroups per 8 rows.  The wavefront culls the decals against the box of its covered
// positions (decal_core.hpp): lane k tests decal k, one vote gives the tile's mask, and a tile no decal touches ends there, having
// read its depth words and G0 texels and written nothing.  No LDS, no barrier: the wavefronts of a workgroup share nothing.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "decal_core.hpp"

namespace cry {

__global__ __launch_bounds__(kDecalThreads) void decal_kernel(const DecalArgs a)
{
    const uint32_t gy = blockIdx.x / a.tilesX, gx = blockIdx.x - gy * a.tilesX;
    const uint32_t px = gx * kDecalGroupW + decal_lane_x(threadIdx.x);
    const uint32_t py = a.row0 + gy * kDecalTile + decal_lane_y(threadIdx.x);
    // no lane leaves before the vote: lane k carries decal k's test whether or not it has a pixel
    const bool in = px < a.W && py < a.rowEnd;
    const uint32_t idx = in ? py * a.W + px : 0u;               // below 2^28
    uint32_t z = 0x00FFFFFFu;
    if (in) z = a.depth[idx];
    const bool covered = (z & 0x00FFFFFFu) < 0x00FFFFFFu;
    DecalTexel T0{ u4{ 0u, 0u, 0u, 0u }, f4a{ 0.0f, 0.0f, 0.0f, 0.0f } };
    if (covered) T0 = decal_load(a.g0, idx, a.h0);
    TileBox box = tile_box_pixel(covered, T0.v);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        TileBox other;
#pragma unroll
        for (int c = 0; c < 3; ++c) { other.lo[c] = __shfl_xor(box.lo[c], off); other.hi[c] = __shfl_xor(box.hi[c], off); }
        box = tile_box_merge(box, other);
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t mask = __ballot(lane < a.n && decal_tile_test(a.decals[lane < a.n ? lane : 0u], box));
    if (mask == 0ull || !covered) return;
    decal_lane(a, idx, T0, mask, [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); });
}

hipError_t launch_decals(const float* view, const float* proj, const uint32_t* depth, void* g0, void* g1, void* g2, uint32_t formatFlags,
                         const crychic_decal* decals, uint32_t nDecals, const crychic_texture* textures, uint32_t nTextures, uint32_t W, uint32_t H,
                         uint32_t row0, uint32_t rows, hipStream_t stream)
{
    const DecalLaunch L = decal_launch(view, proj, depth, g0, g1, g2, formatFlags, decals, nDecals, textures, nTextures, W, H, row0, rows);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(decal_kernel, dim3(L.groups), dim3(kDecalThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
