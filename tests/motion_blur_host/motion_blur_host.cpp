// motion_blur_host.cpp -- csrc/motion_blur_core.hpp built for the host (TEST INFRASTRUCTURE): the launchers' plans and constants and
// the kernels' walk over a one-dimensional grid of workgroups, one 16 x 16 tile and 256 threads each, as motion_blur.hip does it.
// The tile reduction is the walk's own: the threads of a workgroup run one after the other, each folds its key into the running
// maximum, and the last one owns the result (the device: lane exchanges, four LDS words, thread 0).
#include <cstdint>
#include "motion_blur_core.hpp"

static cry::MotionBlurParams params_of(uint32_t shutter, uint32_t samples, uint32_t maxRadius)
{
    cry::MotionBlurParams p = {};
    p.shutter = shutter;
    p.samples = samples;
    p.maxRadius = maxRadius;
    return p;
}

// Returns the number of workgroups walked.
extern "C" uint32_t mbh_velocity(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, uint32_t W, uint32_t H,
                                 uint32_t shutter, uint32_t maxRadius, void* workspace)
{
    using namespace cry;
    const MbVelocityLaunch L = mb_velocity_launch(invViewProj, curViewProj, prevViewProj, depth, W, H, params_of(shutter, 8u, maxRadius), workspace);
    const MbVelocityArgs& a = L.args;
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t ty = g / a.tilesX, tx = g - ty * a.tilesX;
        uint64_t best = 0u;
        const auto reduce = [&best](uint64_t key, uint32_t thread, bool& owner) {
            best = key > best ? key : best;
            owner = thread == kMbThreads - 1u;
            return best;
        };
        for (uint32_t t = 0; t < kMbThreads; ++t) mb_velocity_thread(a, tx, ty, t, reduce);
    }
    return L.groups;
}

extern "C" uint32_t mbh_gather(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t samples,
                               const void* workspace)
{
    using namespace cry;
    const MbGatherLaunch L = mb_gather_launch(in, out, W, H, row0, rows, params_of(128u, samples, 16u), workspace);
    const MbGatherArgs& a = L.args;
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t gy = g / a.tilesX, tx = g - gy * a.tilesX;
        for (uint32_t t = 0; t < kMbThreads; ++t) mb_gather_thread(a, tx, a.tileRow0 + gy, t);
    }
    return L.groups;
}

extern "C" uint64_t mbh_workspace_bytes(uint32_t W, uint32_t H) { return cry::mb_workspace_bytes(W, H); }
