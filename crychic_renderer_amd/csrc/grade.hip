// grade.hip -- crychic_grade: the colour grade of a finished RGBA8 frame through a 3D look-up table.  A
// persistent launch (grade_core.hpp): each workgroup copies the table into LDS -- sized 4 N^3 bytes at the launch, so that a small
// table does not cost occupancy -- and strides over the row range.  Workgroups share nothing: they read `in` and the table and write
// disjoint texels of `out`.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "grade_core.hpp"

namespace cry {

template <bool VEC>
__global__ __launch_bounds__(kGradeThreads) void grade_kernel(const GradeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_lut[];
    grade_stage(a, threadIdx.x, kGradeThreads, s_lut);
    __syncthreads();
    grade_walk<VEC>(a, blockIdx.x, gridDim.x, threadIdx.x, kGradeThreads, s_lut);
}

namespace {
// The compute units of the current device, asked for once per device.
hipError_t grade_cus(uint32_t* cus, int* device)
{
    static int known[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    *device = dev;
    if (e != hipSuccess) return e;
    int n = (dev >= 0 && dev < 64) ? known[dev] : 0;
    if (n == 0) {
        e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
        if (n < 1) n = 1;
        if (dev >= 0 && dev < 64) known[dev] = n;
    }
    *cus = (uint32_t)n;
    return hipSuccess;
}

template <bool VEC>
hipError_t grade_go(const GradeLaunch& L, int dev, hipStream_t stream)
{
    // more than 64 KiB of dynamic LDS has to be announced, once per device; a refusal comes back as an error code, here or from the
    // launch
    static bool announced[64] = {};
    if (L.ldsBytes > 65536u && !(dev >= 0 && dev < 64 && announced[dev])) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&grade_kernel<VEC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(4u * kGradeMaxN * kGradeMaxN * kGradeMaxN));
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) announced[dev] = true;
    }
    hipLaunchKernelGGL(grade_kernel<VEC>, dim3(L.groups), dim3(kGradeThreads), L.ldsBytes, stream, L.args);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_grade(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint8_t* lut, uint32_t N,
                        hipStream_t stream)
{
    (void)H;
    if (rows == 0u) return hipSuccess;
    uint32_t cus = 0u;
    int dev = 0;
    const hipError_t e = grade_cus(&cus, &dev);
    if (e != hipSuccess) return e;
    const GradeLaunch L = grade_launch(in, out, W, row0, rows, lut, N, cus);
    if (L.groups == 0u) return hipSuccess;
    return L.vec ? grade_go<true>(L, dev, stream) : grade_go<false>(L, dev, stream);
}

}  // namespace cry
