// ssr.hip -- crychic_ssr: screen-space reflections of the lit frame, one pass over a finished RGBA8 frame.
// One lane per pixel, an 8 x 8 pixel tile per wavefront, four tiles side by side per workgroup (ssr_core.hpp); a 1-D grid of tilesX
// workgroups per 8 rows, so that neither a very wide nor a very tall frame meets a grid limit.  Lanes share nothing: each reads its
// own texels of `in`, `depth` and the G-buffer, gathers from `depth` along its ray and one texel of `in` at its hit, and writes its
// own texel of `out`.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "ssr_core.hpp"

namespace cry {

__global__ __launch_bounds__(kSsrThreads) void ssr_kernel(const SsrArgs a)
{
    const uint32_t gy = blockIdx.x / a.tilesX, gx = blockIdx.x - gy * a.tilesX;
    const uint32_t px = gx * kSsrGroupW + fog_lane_x(threadIdx.x);
    const uint32_t py = a.row0 + gy * kSsrTile + fog_lane_y(threadIdx.x);
    if (px >= a.W || py >= a.rowEnd) return;
    ssr_pixel(a, px, py, [](bool p) { return __any(p) != 0; });
}

hipError_t launch_ssr(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, float nearZ, const void* g0,
                      const void* g1, const void* g2, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H,
                      uint32_t row0, uint32_t rows, uint32_t formatFlags, const SsrParams& p, hipStream_t stream)
{
    const SsrLaunch L = ssr_launch(proj, viewProj, invViewProj, eye, nearZ, g0, g1, g2, depth, in, out, W, H, row0, rows, formatFlags, p);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(ssr_kernel, dim3(L.groups), dim3(kSsrThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
