// ssr_gloss.hip -- crychic_ssr_glossy: crychic_ssr with the hit colour from a pyramid of the lit frame.  The
// grid, the workgroup and the lane's pixel are ssr.hip's; the pixel's body is ssr_pixel with the glossy policy of ssr_gloss_core.hpp.
// Lanes share nothing: besides what ssr_kernel reads, a lane gathers four texels of one or two levels of the pyramid at its hit.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "ssr_gloss_core.hpp"

namespace cry {

__global__ __launch_bounds__(kSsrThreads) void ssr_gloss_kernel(const SsrGlossArgs a)
{
    const uint32_t gy = blockIdx.x / a.s.tilesX, gx = blockIdx.x - gy * a.s.tilesX;
    const uint32_t px = gx * kSsrGroupW + fog_lane_x(threadIdx.x);
    const uint32_t py = a.s.row0 + gy * kSsrTile + fog_lane_y(threadIdx.x);
    if (px >= a.s.W || py >= a.s.rowEnd) return;
    ssr_pixel(a.s, px, py, [](bool p) { return __any(p) != 0; }, SsrGlossHit{ a });
}

hipError_t launch_ssr_glossy(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, float nearZ, const void* g0,
                             const void* g1, const void* g2, const uint32_t* depth, const uint8_t* in, const void* pyramid, uint8_t* out, uint32_t W,
                             uint32_t H, uint32_t row0, uint32_t rows, uint32_t formatFlags, const SsrParams& p, const SsrGlossParams& g,
                             hipStream_t stream)
{
    const SsrGlossLaunch L = ssr_gloss_launch(ssr_launch(proj, viewProj, invViewProj, eye, nearZ, g0, g1, g2, depth, in, out, W, H, row0, rows, formatFlags, p),
                                              pyramid, g);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(ssr_gloss_kernel, dim3(L.groups), dim3(kSsrThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
