// cube_sh.hip -- crychic_project_cube_sh: the order-2 spherical-harmonics irradiance coefficients of one cube map level (DESIGN.md
// section 16; bodies in cube_sh_core.hpp).  Three short launches on the caller's stream, ordered by the stream alone:
//   zero        28 lanes clear the 64-bit accumulators in the tail (whatever the tail held: no initialisation requirement);
//   accumulate  one lane per texel in a grid-stride loop over a capped grid; a lane keeps the 28 sums in registers, the wavefront
//               adds them by xor shuffles, the workgroup's four waves through LDS, and 28 lanes issue one 64-bit integer atomic add
//               each -- 224 contiguous bytes per workgroup, at most 256 workgroups;
//   finalise    one wavefront: 36 lanes turn the sums into the nine float4 of the coefficient block in double precision.
// No workgroup waits for another, nothing is allocated or read back, and every sum is an integer: the block does not depend on the
// order in which lanes, waves or workgroups arrive.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "cube_sh_core.hpp"

namespace cry {

__global__ __launch_bounds__(64) void cube_sh_zero_kernel(unsigned long long* __restrict__ sums)
{
    if (threadIdx.x < kCubeShSums) sums[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(kCubeShThreads) void cube_sh_accumulate_kernel(const uint32_t* __restrict__ level, uint32_t d,
                                                                            unsigned long long* __restrict__ sums)
{
    __shared__ long long s_part[kCubeShThreads / 64u][kCubeShSums];
    int64_t s[kCubeShSums];
#pragma unroll
    for (uint32_t k = 0; k < kCubeShSums; ++k) s[k] = 0;
    const uint32_t texels = 6u * d * d;                           // d <= 8192: below 2^29, and an index plus the stride below 2^32
    const uint32_t stride = gridDim.x * kCubeShThreads;
    for (uint32_t i = blockIdx.x * kCubeShThreads + threadIdx.x; i < texels; i += stride) cube_sh_accumulate(level, d, i, s);
#pragma unroll
    for (uint32_t k = 0; k < kCubeShSums; ++k) {
        long long v = s[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        s[k] = v;
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < kCubeShSums; ++k) s_part[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < kCubeShSums) {
        long long v = 0;
#pragma unroll
        for (uint32_t w = 0; w < kCubeShThreads / 64u; ++w) v += s_part[w][threadIdx.x];
        atomicAdd(&sums[threadIdx.x], (unsigned long long)v);   // two's complement: the unsigned add is the signed one
    }
}

__global__ __launch_bounds__(64) void cube_sh_finalise_kernel(const long long* __restrict__ sums, float* __restrict__ coeffs)
{
    if (threadIdx.x < 36u) coeffs[threadIdx.x] = cube_sh_coefficient(reinterpret_cast<const int64_t*>(sums), threadIdx.x);
}

hipError_t launch_cube_sh(const uint8_t* level, uint32_t d, void* tail, hipStream_t stream)
{
    float* coeffs = static_cast<float*>(tail);
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(tail) + kCubeShCoeffBytes);
    const uint32_t texels = 6u * d * d;
    uint32_t blocks = (texels + kCubeShThreads - 1u) / kCubeShThreads;
    if (blocks > kCubeShMaxBlocks) blocks = kCubeShMaxBlocks;
    hipLaunchKernelGGL(cube_sh_zero_kernel, dim3(1), dim3(64), 0, stream, sums);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(cube_sh_accumulate_kernel, dim3(blocks), dim3(kCubeShThreads), 0, stream, reinterpret_cast<const uint32_t*>(level), d, sums);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(cube_sh_finalise_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const long long*>(sums), coeffs);
    return hipGetLastError();
}

// crychic_set_cube_probe_volume: the probe volume of the box-projected reflection lookup into tail bytes
// [CRYCHIC_CUBE_PROBE_OFFSET, + CRYCHIC_CUBE_PROBE_BYTES).  The twelve floats arrive by value in the kernel's arguments; lane k < 12
// stores dword k with an ordinary vector store.
struct ProbeVolumeArgs { float v[12]; };
__global__ __launch_bounds__(64) void cube_probe_volume_kernel(float* __restrict__ probe, ProbeVolumeArgs a)
{
    if (threadIdx.x < 12u) {
        float x = a.v[0];
#pragma unroll
        for (uint32_t k = 1; k < 12u; ++k) x = threadIdx.x == k ? a.v[k] : x;      // selects: the arguments stay in scalar registers
        probe[threadIdx.x] = x;
    }
}

hipError_t launch_cube_probe_volume(void* tail, const float pos[3], const float boxMin[3], const float boxMax[3], hipStream_t stream)
{
    ProbeVolumeArgs a;
    for (int k = 0; k < 3; ++k) { a.v[k] = pos[k]; a.v[4 + k] = boxMin[k]; a.v[8 + k] = boxMax[k]; }
    a.v[3] = a.v[7] = a.v[11] = 0.0f;
    float* probe = reinterpret_cast<float*>(static_cast<uint8_t*>(tail) + CRYCHIC_CUBE_PROBE_OFFSET);
    hipLaunchKernelGGL(cube_probe_volume_kernel, dim3(1), dim3(64), 0, stream, probe, a);
    return hipGetLastError();
}

}  // namespace cry
