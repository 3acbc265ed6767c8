// fog.hip -- crychic_fog: volumetric fog with sun shafts through the cascade maps, one pass over a finished RGBA8 frame (DESIGN.md
// section 20).  One lane per pixel, an 8 x 8 pixel tile per wavefront, four tiles side by side per workgroup (fog_core.hpp); a 1-D grid
// of tilesX workgroups per 8 rows, so that neither a very wide nor a very tall frame meets a grid limit.  Lanes share nothing: each
// reads its own texel of `in` and `depth`, gathers from the maps and writes its own texel of `out`.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "fog_core.hpp"

namespace cry {

__global__ __launch_bounds__(kFogThreads) void fog_kernel(const FogArgs a)
{
    const uint32_t gy = blockIdx.x / a.tilesX, gx = blockIdx.x - gy * a.tilesX;
    const uint32_t px = gx * kFogGroupW + fog_lane_x(threadIdx.x);
    const uint32_t py = a.row0 + gy * kFogTile + fog_lane_y(threadIdx.x);
    if (px >= a.W || py >= a.rowEnd) return;
    fog_pixel(a, px, py, [](bool p) { return __any(p) != 0; });
}

hipError_t launch_fog(const float* invViewProj, const float* eye, const float (*shadowTransforms)[16], const uint32_t* depth,
                      const uint32_t* const* maps, uint32_t dim, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                      uint32_t rows, const FogParams& p, hipStream_t stream)
{
    const FogLaunch L = fog_launch(invViewProj, eye, shadowTransforms, depth, maps, dim, in, out, W, H, row0, rows, p);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(fog_kernel, dim3(L.groups), dim3(kFogThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
