// taa.hip -- crychic_taa: the finished RGBA8 frame blended into a history reprojected through the depth plane.
// One lane per pixel, an 8 x 8 pixel tile per wavefront, four tiles side by side per workgroup (taa_core.hpp); a 1-D grid of tilesX
// workgroups per 8 rows, so that neither a very wide nor a very tall frame meets a grid limit.  Lanes share nothing.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "taa_core.hpp"

namespace cry {

__global__ __launch_bounds__(kTaaThreads) void taa_kernel(const TaaArgs a)
{
    const uint32_t gy = blockIdx.x / a.tilesX, gx = blockIdx.x - gy * a.tilesX;
    const uint32_t px = gx * kTaaGroupW + taa_lane_x(threadIdx.x);
    const uint32_t py = a.row0 + gy * kTaaTile + taa_lane_y(threadIdx.x);
    if (px >= a.W || py >= a.rowEnd) return;
    taa_pixel(a, px, py, [](bool p) { return __any(p) != 0; });
}

hipError_t launch_taa(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, const uint8_t* in,
                      const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                      const TaaParams& p, hipStream_t stream)
{
    const TaaLaunch L = taa_launch(invViewProj, curViewProj, prevViewProj, depth, in, historyIn, historyOut, out, W, H, row0, rows, p);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(taa_kernel, dim3(L.groups), dim3(kTaaThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
