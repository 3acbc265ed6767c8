// env_brdf.hip -- crychic_build_env_brdf: the 32 x 32 environment BRDF table of the split-sum specular term (DESIGN.md section 17;
// bodies in env_brdf_core.hpp).  One launch on the caller's stream: one wavefront per texel, four per workgroup, 256 workgroups.  A
// lane takes four xi times the sixteen phi, the wavefront adds the two 64-bit sums by xor shuffles, and lane 0 stores the texel.
// Nothing is allocated or read back and no wavefront waits for another; the sums are integers, so the table does not depend on which
// lane took which sample.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "env_brdf_core.hpp"

namespace cry {

constexpr uint32_t kEnvBrdfThreads = 256u;
static_assert(kEnvBrdfXi % 64u == 0u && (kEnvBrdfDim * kEnvBrdfDim) % (kEnvBrdfThreads / 64u) == 0u, "whole wavefronts, whole workgroups");

__global__ __launch_bounds__(kEnvBrdfThreads) void env_brdf_kernel(uint32_t* __restrict__ table)
{
    const uint32_t texel = blockIdx.x * (kEnvBrdfThreads / 64u) + (threadIdx.x >> 6);      // < 1024 by the grid
    const uint32_t lane = threadIdx.x & 63u;
    const EnvBrdfTexel T = env_brdf_texel(texel / kEnvBrdfDim, texel % kEnvBrdfDim);
    int64_t sa = 0, sb = 0;
    for (uint32_t m = 0; m < kEnvBrdfXi / 64u; ++m) env_brdf_accumulate(T, lane * (kEnvBrdfXi / 64u) + m, sa, sb);
    long long a = sa, b = sb;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    if (lane == 0u) table[texel] = env_brdf_pack(a, b);
}

hipError_t launch_env_brdf(void* table, hipStream_t stream)
{
    hipLaunchKernelGGL(env_brdf_kernel, dim3(kEnvBrdfDim * kEnvBrdfDim / (kEnvBrdfThreads / 64u)), dim3(kEnvBrdfThreads), 0, stream,
                       static_cast<uint32_t*>(table));
    return hipGetLastError();
}

}  // namespace cry
