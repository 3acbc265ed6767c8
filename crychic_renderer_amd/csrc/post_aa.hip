// post_aa.hip -- crychic_antialias: the post-process anti-aliasing pass over a finished RGBA8 frame.  One
// workgroup per 64 x 32 output tile (post_aa_core.hpp): the tile's lumas with a 16-texel apron in LDS, step 1 per texel, then steps
// 2 .. 7 over the tile's list of edge texels.
// Workgroups share nothing: they read `in` and write disjoint texels of `out`.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "post_aa_core.hpp"

namespace cry {

template <bool VEC>
__global__ __launch_bounds__(kAaThreads) void post_aa_kernel(const PostAaArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_luma[kAaLdsTexels];
    __shared__ PostAaEdgeList s_edges;
    PostAaLane lane;
    if (threadIdx.x == 0) s_edges.count = 0u;
    post_aa_fill<VEC>(a, blockIdx.x, blockIdx.y, threadIdx.x, s_luma, lane);
    __syncthreads();
    post_aa_detect<VEC>(a, blockIdx.x, blockIdx.y, threadIdx.x, s_luma, lane, &s_edges);
    __syncthreads();
    post_aa_edges(a, blockIdx.x, blockIdx.y, threadIdx.x, s_luma, &s_edges, [](bool p) { return __any(p) != 0; });
}

hipError_t launch_post_aa(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const PostAaParams& p,
                          hipStream_t stream)
{
    const PostAaLaunch L = post_aa_launch(in, out, W, H, row0, rows, p);
    if (L.tilesY == 0u) return hipSuccess;
    const dim3 grid(L.tilesX, L.tilesY);
    if (L.vec) hipLaunchKernelGGL(post_aa_kernel<true>, grid, dim3(kAaThreads), 0, stream, L.args);
    else hipLaunchKernelGGL(post_aa_kernel<false>, grid, dim3(kAaThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
