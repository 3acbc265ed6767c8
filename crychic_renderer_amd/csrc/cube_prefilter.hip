// cube_prefilter.hip -- crychic_prefilter_cube_chain: levels 1 .. levels - 1 of a cube map chain convolved with the GGX lobe of
// roughness k / (levels - 1).  One launch per level, one lane per output texel (cube_prefilter_core.hpp); the
// level's sample table travels by value in the kernarg segment, so a table entry is a scalar load and a launch needs no device
// buffer of its own: nothing is allocated, uploaded or kept alive, and the launches can be captured into a graph as they are.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "cube_prefilter_core.hpp"

namespace cry {

__global__ __launch_bounds__(kCubePrefilterThreads) void cube_prefilter_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dstLevel,
                                                                               uint32_t dim, uint32_t levels, uint32_t d, CubePrefilterTable tab)
{
    cube_prefilter_thread(src, dstLevel, dim, levels, d, blockIdx.x * kCubePrefilterThreads + threadIdx.x, tab);
}

hipError_t launch_cube_prefilter(const uint8_t* src, uint8_t* dst, uint32_t dim, uint32_t levels, hipStream_t stream)
{
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* level = reinterpret_cast<uint32_t*>(dst);
    if (hipError_t e = hipMemcpyAsync(dst, src, (size_t)6u * dim * dim * 4u, hipMemcpyDeviceToDevice, stream)) return e;
    for (uint32_t k = 1; k < levels; ++k) {
        const uint32_t dPrev = cube_level_dim(dim, k - 1u), d = cube_level_dim(dim, k);
        level += (size_t)6u * dPrev * dPrev;
        CubePrefilterTable tab;
        if (crychic_cube_prefilter_samples(dim, levels, k, tab.s, &tab.count, &tab.rcpW) != 0) return hipErrorInvalidValue;
        const uint32_t texels = 6u * d * d;
        hipLaunchKernelGGL(cube_prefilter_kernel, dim3((texels + kCubePrefilterThreads - 1u) / kCubePrefilterThreads), dim3(kCubePrefilterThreads), 0,
                           stream, s, level, dim, levels, d, tab);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace cry
