// cube_mips.hip -- crychic_generate_cube_mips: the mip chain of an RGBA8 cube map, built on the device, in place (DESIGN.md
// section 14).  One workgroup per 64 x 64 tile of one face of the launch's input level, up to six levels per launch
// (cube_mips_core.hpp); levels beyond a tile's pyramid come from a further launch of the same kernel on the last level written.
// Workgroups of one launch share nothing: they read the input level and write disjoint texels of the levels after it.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "cube_mips_core.hpp"

namespace cry {

template <bool VEC>
__global__ __launch_bounds__(kCubeMipThreads) void cube_mips_kernel(uint32_t* __restrict__ levelIn, uint32_t dIn, uint32_t nLevels)
{
    __shared__ uint32_t s_tile[kCubeMipTileWords];
    cube_mips_tile<VEC>(levelIn, dIn, nLevels, blockIdx.z, blockIdx.x, blockIdx.y, threadIdx.x, s_tile, [] { __syncthreads(); });
}

hipError_t launch_cube_mips(uint8_t* chain, uint32_t dim, uint32_t levels, hipStream_t stream)
{
    for (uint32_t i = 0; i < cube_mips_launches(levels); ++i) {
        const CubeMipLaunch L = cube_mips_launch(chain, dim, levels, i);
        const dim3 grid(L.tiles, L.tiles, 6);
        if (L.vec) hipLaunchKernelGGL(cube_mips_kernel<true>, grid, dim3(kCubeMipThreads), 0, stream, L.levelIn, L.dIn, L.nLevels);
        else hipLaunchKernelGGL(cube_mips_kernel<false>, grid, dim3(kCubeMipThreads), 0, stream, L.levelIn, L.dIn, L.nLevels);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace cry
