// taa_upscale.hip -- crychic_taa_upscale: jittered RGBA8 frames of the render size accumulated into a history of the display size,
// reprojected through the depth plane.  One lane per output pixel, an 8 x 8 output tile per wavefront, four
// tiles side by side per workgroup (taa_upscale_core.hpp); a 1-D grid of tilesX workgroups per 8 output rows, as in taa.hip.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "taa_upscale_core.hpp"

namespace cry {

__global__ __launch_bounds__(kTaaThreads) void taa_upscale_kernel(const TaaUpscaleArgs a)
{
    const uint32_t gy = blockIdx.x / a.tilesX, gx = blockIdx.x - gy * a.tilesX;
    const uint32_t ox = gx * kTaaGroupW + taa_lane_x(threadIdx.x);
    const uint32_t oy = a.row0 + gy * kTaaTile + taa_lane_y(threadIdx.x);
    if (ox >= a.Wo || oy >= a.rowEnd) return;
    taa_upscale_pixel(a, ox, oy, [](bool p) { return __any(p) != 0; });
}

hipError_t launch_taa_upscale(const float* invViewProj, const float* curViewProj, const float* prevViewProj, float jx, float jy, const uint32_t* depth,
                              const uint8_t* in, uint32_t Wi, uint32_t Hi, const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t Wo,
                              uint32_t Ho, uint32_t row0, uint32_t rows, const TaaUpscaleParams& p, hipStream_t stream)
{
    const TaaUpscaleLaunch L = taa_upscale_launch(invViewProj, curViewProj, prevViewProj, jx, jy, depth, in, Wi, Hi, historyIn, historyOut, out, Wo, Ho,
                                                  row0, rows, p);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(taa_upscale_kernel, dim3(L.groups), dim3(kTaaThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
