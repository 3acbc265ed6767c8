// sharpen.hip -- crychic_sharpen: contrast-adaptive sharpening of a finished RGBA8 frame.  A streaming
// five-tap stencil without LDS (sharpen_core.hpp): in the wide kernel a lane owns four pixels of a row and walks a strip of rows with
// a three-row window in registers; the pixels left and right of its four come from the neighbouring lanes by two lane permutes.
// Workgroups share nothing: they read `in` and write disjoint pixels of `out`.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "sharpen_core.hpp"

namespace cry {

namespace {
// The pixels left and right of the lane's quad of row R.  Every lane of the wavefront gets here together.
__device__ __forceinline__ void sharpen_exchange(const SharpenLane& L, SharpenRow& R)
{
    const int below = (int)(((L.lane + kSharpenWave - 1u) & (kSharpenWave - 1u)) << 2), above = (int)(((L.lane + 1u) & (kSharpenWave - 1u)) << 2);
    const uint32_t fromBelow = (uint32_t)__builtin_amdgcn_ds_bpermute(below, (int)sharpen_exchange_up(R));
    const uint32_t fromAbove = (uint32_t)__builtin_amdgcn_ds_bpermute(above, (int)sharpen_exchange_down(R));
    sharpen_exchange_take(L, R, fromBelow, fromAbove);
}
}  // namespace

// The row after next is asked for before the current one is worked out, so its latency lies behind a row's arithmetic; the last two
// trips ask for a row they do not use (clamped to the frame) rather than branch around the load, which would make the row wait.
__global__ __launch_bounds__(kSharpenThreads) void sharpen_wide_kernel(const SharpenArgs a)
{
    if (sharpen_wave_idle(a, blockIdx.x, threadIdx.x)) return;      // the whole wavefront: no permute is left waiting
    const SharpenLane L = sharpen_lane(a, blockIdx.x, threadIdx.x);
    SharpenPx4 up = sharpen_load_row(a, L, sharpen_row_above(L.y0)).px;
    SharpenRow mid = sharpen_load_row(a, L, L.y0);
    SharpenRow dn = sharpen_load_row(a, L, sharpen_row_below(a, L.y0));
    sharpen_exchange(L, mid);
    sharpen_exchange(L, dn);
    for (uint32_t y = L.y0; y < L.y1; ++y) {
        SharpenRow next = sharpen_load_row(a, L, sharpen_row_below(a, y + 1u));
        sharpen_store(a, L, y, sharpen_quad(a, up, mid, dn.px));
        sharpen_exchange(L, next);
        up = mid.px;
        mid = dn;
        dn = next;
    }
}

__global__ __launch_bounds__(kSharpenThreads) void sharpen_narrow_kernel(const SharpenArgs a)
{
    const uint32_t i = blockIdx.x * kSharpenThreads + threadIdx.x;
    if (i < a.rows * a.W) sharpen_narrow(a, i);
}

hipError_t launch_sharpen(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const SharpenParams& p,
                          hipStream_t stream)
{
    if (rows == 0u) return hipSuccess;
    const SharpenLaunch L = sharpen_launch(in, out, W, H, row0, rows, p.strength, p.limit);
    if (L.wide) hipLaunchKernelGGL(sharpen_wide_kernel, dim3(L.groups), dim3(kSharpenThreads), 0, stream, L.args);
    else hipLaunchKernelGGL(sharpen_narrow_kernel, dim3(L.groups), dim3(kSharpenThreads), 0, stream, L.args);
    return hipGetLastError();
}

}  // namespace cry
