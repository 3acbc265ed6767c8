// bloom.hip -- crychic_bloom: threshold, binomial pyramid and additive composite over a finished RGBA8 frame.
// Three kernels around the bodies of bloom_core.hpp: the downsample (instantiated for the frame, which it weighs on load, and for a
// pyramid level), the in-place unwind of one level and the composite.  Every dependency between levels is a launch boundary on the
// stream: no workgroup waits on another, and the workgroups of one launch write disjoint texels.  All grids are one-dimensional.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "bloom_core.hpp"

namespace cry {

template <bool First>
__global__ __launch_bounds__(kBloomThreads) void bloom_down_kernel(const BloomDownArgs a)
{
    __shared__ BloomTexel s_win[kBloomWinTexels];
    __shared__ uint32_t s_sums[kBloomRowSums];
    __shared__ uint32_t s_any[kBloomWaves];
    const uint32_t tileY = blockIdx.x / a.tilesX, tileX = blockIdx.x - tileY * a.tilesX;
    const uint32_t any = bloom_down_stage<First>(a, tileX, tileY, threadIdx.x, s_win);
    const uint32_t waveAny = __any((int)(any != 0u)) ? 1u : 0u;         // the vote: did this wavefront stage anything but zeros
    if ((threadIdx.x & 63u) == 0u) s_any[threadIdx.x >> 6] = waveAny;
    __syncthreads();
    uint32_t tileAny = 0u;
    for (uint32_t w = 0; w < kBloomWaves; ++w) tileAny |= s_any[w];
    if (__builtin_amdgcn_readfirstlane((int)tileAny) == 0) {            // uniform over the workgroup: no barrier is skipped by a part of it
        bloom_down_zero(a, tileX, tileY, threadIdx.x);
        return;
    }
    bloom_down_rows(threadIdx.x, s_win, s_sums);
    __syncthreads();
    bloom_down_columns(a, tileX, tileY, threadIdx.x, s_sums);
}

__global__ __launch_bounds__(kBloomThreads) void bloom_unwind_kernel(const BloomUnwindArgs a)
{
    bloom_unwind(a, blockIdx.x * kBloomThreads + threadIdx.x);
}

__global__ __launch_bounds__(kBloomThreads) void bloom_composite_kernel(const BloomCompositeArgs a)
{
    const BloomCompositeLane l = bloom_composite_eval(a, blockIdx.x * kBloomThreads + threadIdx.x);
    // in place, a wavefront that added nothing to any pixel has nothing to store
    if (a.inPlace && !__any((int)(l.added != 0u))) return;
    bloom_composite_store(a, l);
}

hipError_t launch_bloom_pyramid(const uint8_t* in, uint32_t W, uint32_t H, const BloomParams& p, void* workspace, hipStream_t stream)
{
    const BloomPlan plan = bloom_plan(W, H, p.levels);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    for (uint32_t k = 1; k <= plan.nEff; ++k) {
        if (k == 1u) {
            const BloomDownLaunch L = bloom_down_launch(in, ws + plan.off[1], W, H, &p);
            hipLaunchKernelGGL(bloom_down_kernel<true>, dim3(L.groups), dim3(kBloomThreads), 0, stream, L.args);
        } else {
            const BloomDownLaunch L = bloom_down_launch(ws + plan.off[k - 1u], ws + plan.off[k], plan.w[k - 1u], plan.h[k - 1u], nullptr);
            hipLaunchKernelGGL(bloom_down_kernel<false>, dim3(L.groups), dim3(kBloomThreads), 0, stream, L.args);
        }
    }
    for (uint32_t k = plan.nEff - 1u; k >= 1u; --k) {
        const BloomUnwindArgs a = bloom_unwind_args(ws + plan.off[k], ws + plan.off[k + 1u], plan.w[k], plan.h[k], p.scatter);
        hipLaunchKernelGGL(bloom_unwind_kernel, dim3((a.n + kBloomThreads - 1u) / kBloomThreads), dim3(kBloomThreads), 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_bloom_composite(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const BloomParams& p,
                                  const void* workspace, hipStream_t stream)
{
    const BloomPlan plan = bloom_plan(W, H, p.levels);
    const BloomCompositeLaunch L = bloom_composite_launch(in, out, static_cast<const uint8_t*>(workspace) + plan.off[1], W, H, row0, rows, p.intensity);
    if (L.groups == 0u) return hipSuccess;
    hipLaunchKernelGGL(bloom_composite_kernel, dim3(L.groups), dim3(kBloomThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
