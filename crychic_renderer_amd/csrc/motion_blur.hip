// motion_blur.hip -- crychic_motion_blur: camera-motion blur of the finished RGBA8 frame.  Two launches, each a
// 1-D grid of one 256-thread workgroup per 16 x 16 pixel tile (motion_blur_core.hpp): the velocity kernel writes the velocity plane and
// reduces each tile's largest key, the gather kernel reads the nine tile words around its tile and gathers along the dominant velocity.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "motion_blur_core.hpp"

namespace cry {

// The tile's largest key: xor exchanges across the 64 lanes of a wavefront, then four keys through LDS.  Thread 0 owns the result.
__device__ __forceinline__ uint64_t mb_reduce_tile(uint64_t key, uint32_t thread, bool& owner, uint64_t* waveKeys)
{
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const uint64_t other = __shfl_xor((unsigned long long)key, step, 64);
        key = other > key ? other : key;
    }
    if ((thread & 63u) == 0u) waveKeys[thread >> 6] = key;
    __syncthreads();
    owner = thread == 0u;
    if (!owner) return 0u;
    const uint64_t k01 = waveKeys[0] > waveKeys[1] ? waveKeys[0] : waveKeys[1], k23 = waveKeys[2] > waveKeys[3] ? waveKeys[2] : waveKeys[3];
    return k01 > k23 ? k01 : k23;
}

__global__ __launch_bounds__(kMbThreads) void motion_blur_velocity_kernel(const MbVelocityArgs a)
{
    __shared__ uint64_t waveKeys[kMbThreads / 64u];
    const uint32_t ty = blockIdx.x / a.tilesX, tx = blockIdx.x - ty * a.tilesX;
    mb_velocity_thread(a, tx, ty, threadIdx.x, [&](uint64_t key, uint32_t thread, bool& owner) { return mb_reduce_tile(key, thread, owner, waveKeys); });
}

__global__ __launch_bounds__(kMbThreads) void motion_blur_gather_kernel(const MbGatherArgs a)
{
    const uint32_t gy = blockIdx.x / a.tilesX, tx = blockIdx.x - gy * a.tilesX;
    mb_gather_thread(a, tx, a.tileRow0 + gy, threadIdx.x);
}

hipError_t launch_motion_blur_velocity(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, uint32_t W,
                                       uint32_t H, const MotionBlurParams& p, void* workspace, hipStream_t stream)
{
    const MbVelocityLaunch L = mb_velocity_launch(invViewProj, curViewProj, prevViewProj, depth, W, H, p, workspace);
    hipLaunchKernelGGL(motion_blur_velocity_kernel, dim3(L.groups), dim3(kMbThreads), 0, stream, L.args);
    return hipGetLastError();
}

hipError_t launch_motion_blur_gather(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const MotionBlurParams& p,
                                     const void* workspace, hipStream_t stream)
{
    const MbGatherLaunch L = mb_gather_launch(in, out, W, H, row0, rows, p, workspace);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(motion_blur_gather_kernel, dim3(L.groups), dim3(kMbThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
