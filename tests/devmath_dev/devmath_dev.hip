// devmath_dev.hip -- TEST HARNESS ONLY.  Evaluates one primitive of csrc/devmath.hpp per element ON THE DEVICE, so that the
// `__HIP_DEVICE_COMPILE__` branches the host build never compiles (v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 + correction, v_med3_f32,
// v_mul_u32_u24) and everything the amdgcn back end lowers differently from x86 (rintf, ldexpf, floorf, float -> int conversions,
// fminf / fmaxf on NaN, the constant table, _Float16) can be compared with the oracle bit for bit.  Built by
// tests/devmath_dev_lib.py with the product's own flag set (crychic_renderer_amd.build.FLAGS).  Nothing in the product loads it.
//
// One C entry in the style of or_eval_array / hs_eval_array; the kinds are devmath_eval.hpp's.  Every kind has a kernel of its own
// (the kind is a template argument: straight-line code, as where the product inlines the primitive), one element per thread.
#include <hip/hip_runtime.h>
#include "../hostsim/devmath_eval.hpp"
#include <utility>

namespace {

constexpr int kKinds = 52;
constexpr size_t kMaxElements = (size_t)1 << 24;

template <int KIND>
__global__ __launch_bounds__(256) void eval_kernel(uint32_t n, const float* __restrict__ in, const float* __restrict__ in2, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = cry::devmath_eval(KIND, in[i], in2[i]);
}

using Launch = void (*)(uint32_t, const float*, const float*, uint32_t*);
template <int KIND>
void launch(uint32_t n, const float* in, const float* in2, uint32_t* out)
{
    hipLaunchKernelGGL(eval_kernel<KIND>, dim3((n + 255u) / 256u), dim3(256), 0, 0, n, in, in2, out);
}
template <int... K>
Launch pick(int kind, std::integer_sequence<int, K...>)
{
    static const Launch table[] = { &launch<K>... };
    return table[kind];
}

}  // namespace

extern "C" {

// out[i] = kind(in[i], in2[i]) for i < n; all three are HOST pointers to n 32-bit words.  Returns the HIP error code (0: done):
// hipErrorInvalidValue for a kind the harness does not have, n == 0 or n > 2^24, a null pointer.  Never aborts; whatever it
// allocated is freed on every path.
int dm_eval_array(int kind, size_t n, const float* in, const float* in2, float* out)
{
    if (!cry::devmath_eval_has(kind) || kind >= kKinds || n == 0 || n > kMaxElements || !in || !in2 || !out) return (int)hipErrorInvalidValue;
    const size_t bytes = n * sizeof(float);
    float *dIn = nullptr, *dIn2 = nullptr;
    uint32_t* dOut = nullptr;
    hipError_t e = hipMalloc(&dIn, bytes);
    if (e == hipSuccess) e = hipMalloc(&dIn2, bytes);
    if (e == hipSuccess) e = hipMalloc(&dOut, bytes);
    if (e == hipSuccess) e = hipMemcpy(dIn, in, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dIn2, in2, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dOut, 0, bytes);
    if (e == hipSuccess) {
        pick(kind, std::make_integer_sequence<int, kKinds>{})((uint32_t)n, dIn, dIn2, dOut);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dOut, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(dIn);
    (void)hipFree(dIn2);
    (void)hipFree(dOut);
    return (int)e;
}

int dm_max_elements_log2(void) { return 24; }

}  // extern "C"
