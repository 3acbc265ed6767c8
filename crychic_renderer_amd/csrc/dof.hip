// dof.hip -- crychic_dof: depth of field over a finished RGBA8 frame from its D24 depth plane.  One workgroup
// per 64 x 16 output tile (dof_core.hpp): the tile with an apron of R texels in LDS, each texel with its circle of confusion, then up
// to 197 taps per pixel out of that window with no memory traffic in the loop.  A 1-D grid of tilesX workgroups per 16 rows, so that
// neither a very wide nor a very tall frame meets a grid limit.  Workgroups share nothing: they read `in` and `depth` and write
// disjoint texels of `out`.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "dof_core.hpp"

namespace cry {

__global__ __launch_bounds__(kDofThreads) void dof_kernel(const DofArgs a)
{
    // exactly 40 KiB, four workgroups to a CU's 160 KiB: a wavefront's maximum goes into the unused fourth dword of window texel 64 w,
    // not into a second array.  Thread 64 w is the only one that ever stages that texel (dof_stage: i = t first), and it does so
    // before this store in its own program order; the tap loop never looks at the fourth dword.
    __shared__ DofTexel s_win[kDofLdsTexels];
    const uint32_t tileY = blockIdx.x / a.tilesX, tileX = blockIdx.x - tileY * a.tilesX;
    uint32_t m = dof_stage(a, tileX, tileY, threadIdx.x, s_win);
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t n = (uint32_t)__shfl_xor((int)m, o);
        m = n > m ? n : m;
    }
    if ((threadIdx.x & 63u) == 0u) s_win[threadIdx.x][3] = m;
    __syncthreads();
    uint32_t cmax = 0u;
    for (uint32_t w = 0; w < kDofWaves; ++w) {
        const uint32_t v = s_win[64u * w][3];
        cmax = v > cmax ? v : cmax;
    }
    dof_gather(a, tileX, tileY, threadIdx.x, s_win, (uint32_t)__builtin_amdgcn_readfirstlane((int)cmax));
}

hipError_t launch_dof(const float* proj, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                      uint32_t rows, const DofParams& p, hipStream_t stream)
{
    const DofLaunch L = dof_launch(proj, depth, in, out, W, H, row0, rows, p);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(dof_kernel, dim3(L.groups), dim3(kDofThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
