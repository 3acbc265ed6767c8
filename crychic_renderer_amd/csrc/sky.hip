// sky.hip -- crychic_render_sky: a single-scattering atmosphere into level 0 of a cube map.  One lane per
// texel, an 8 x 8 texel tile per wavefront, four tiles side by side per workgroup (sky_core.hpp); a 1-D grid of groupsPerFace
// workgroups per face.  Lanes share nothing and read no memory: each marches its own ray and writes its own texel.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "sky_core.hpp"

namespace cry {

__global__ __launch_bounds__(kSkyThreads) void sky_kernel(const SkyArgs a)
{
    const uint32_t f = blockIdx.x / a.groupsPerFace, g = blockIdx.x - f * a.groupsPerFace;
    const uint32_t gy = g / a.tilesX, gx = g - gy * a.tilesX;
    const uint32_t x = gx * kSkyGroupW + sky_lane_x(threadIdx.x);
    const uint32_t y = gy * kSkyTile + sky_lane_y(threadIdx.x);
    if (x >= a.dim || y >= a.dim) return;
    const uint32_t face = a.face0 + f;              // < 6 by the grid
    // face * dim^2 + y * dim + x < 6 * 8192^2 < 2^29
    a.cube[(face * a.dim + y) * a.dim + x] = sky_texel(a.k, face, x, y, a.rd, [](bool p) { return __any(p) != 0; });
}

hipError_t launch_sky(uint8_t* cube, uint32_t dim, uint32_t face0, uint32_t faces, const SkyParams& p, hipStream_t stream)
{
    const SkyLaunch L = sky_launch(cube, dim, face0, faces, p);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(sky_kernel, dim3(L.groups), dim3(kSkyThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
