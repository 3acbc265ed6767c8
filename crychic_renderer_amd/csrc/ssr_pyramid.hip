// ssr_pyramid.hip -- crychic_ssr_pyramid: the binomial pyramid of a finished RGBA8 frame that crychic_ssr_glossy reads (DESIGN.md
// section 31).  One kernel around the bodies of ssr_pyramid_core.hpp, one launch per level: level k + 1 depends on all of level k, and
// that dependency is the launch boundary on the stream.  No workgroup waits on another, the workgroups of one launch write disjoint
// texels, and the grid is one-dimensional.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "ssr_pyramid_core.hpp"

namespace cry {

__global__ __launch_bounds__(kSsrPyrThreads) void ssr_pyramid_kernel(const SsrPyrArgs a)
{
    __shared__ uint32_t s_win[kSsrPyrWinTexels];
    __shared__ SsrPyrSum s_sums[kSsrPyrRowSums];
    const uint32_t tileY = blockIdx.x / a.tilesX, tileX = blockIdx.x - tileY * a.tilesX;
    ssr_pyr_stage(a, tileX, tileY, threadIdx.x, s_win);
    __syncthreads();
    ssr_pyr_rows(threadIdx.x, s_win, s_sums);
    __syncthreads();
    ssr_pyr_columns(a, tileX, tileY, threadIdx.x, s_sums);
}

hipError_t launch_ssr_pyramid(const uint8_t* in, uint32_t W, uint32_t H, uint32_t levels, void* workspace, hipStream_t stream)
{
    const SsrPyramidPlan plan = ssr_pyramid_plan(W, H, levels);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    for (uint32_t k = 1; k <= plan.nEff; ++k) {
        const void* src = k == 1u ? static_cast<const void*>(in) : ws + plan.off[k - 1u];
        const SsrPyrLaunch L = ssr_pyr_launch(src, ws + plan.off[k], plan.w[k - 1u], plan.h[k - 1u]);
        hipLaunchKernelGGL(ssr_pyramid_kernel, dim3(L.groups), dim3(kSsrPyrThreads), 0, stream, L.args);
    }
    return hipGetLastError();
}

}  // namespace cry
