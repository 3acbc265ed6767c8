// ssr_gloss_host.cpp -- csrc/ssr_pyramid_core.hpp and csrc/ssr_gloss_core.hpp built for the host (TEST INFRASTRUCTURE): the launchers'
// plans and the kernels' walks over their one-dimensional grids of workgroups, 256 threads each, as ssr_pyramid_kernel and
// ssr_gloss_kernel do them.  A barrier is the end of a loop over the workgroup's threads; the wave vote is the lane's own predicate
// (the votes only skip work: ssr_gloss_core.hpp).
#include <cstdint>
#include <cstring>
#include "ssr_gloss_core.hpp"

// Levels 1 .. n_eff of `in`'s pyramid into `workspace`.  Returns the number of workgroups walked over all levels.
extern "C" uint32_t ssgh_pyramid(const uint8_t* in, uint32_t W, uint32_t H, uint32_t levels, uint8_t* workspace)
{
    using namespace cry;
    const SsrPyramidPlan plan = ssr_pyramid_plan(W, H, levels);
    static uint32_t win[kSsrPyrWinTexels];
    static SsrPyrSum sums[kSsrPyrRowSums];
    uint32_t groups = 0;
    for (uint32_t k = 1; k <= plan.nEff; ++k) {
        const void* src = k == 1u ? static_cast<const void*>(in) : workspace + plan.off[k - 1u];
        const SsrPyrLaunch L = ssr_pyr_launch(src, workspace + plan.off[k], plan.w[k - 1u], plan.h[k - 1u]);
        const SsrPyrArgs& a = L.args;
        for (uint32_t g = 0; g < L.groups; ++g) {
            const uint32_t tileY = g / a.tilesX, tileX = g - tileY * a.tilesX;
            std::memset(win, 0xCD, sizeof win);
            std::memset(sums, 0xCD, sizeof sums);
            for (uint32_t t = 0; t < kSsrPyrThreads; ++t) ssr_pyr_stage(a, tileX, tileY, t, win);
            for (uint32_t t = 0; t < kSsrPyrThreads; ++t) ssr_pyr_rows(t, win, sums);
            for (uint32_t t = 0; t < kSsrPyrThreads; ++t) ssr_pyr_columns(a, tileX, tileY, t, sums);
        }
        groups += L.groups;
    }
    return groups;
}

// params: the eight words of crychic_ssr_params; gloss: the four of crychic_ssr_gloss_params (tests/ssr_gloss_lib.py).  Returns the
// number of workgroups walked.
extern "C" uint32_t ssgh_glossy(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, const float* nearZ,
                                const void* g0, const void* g1, const void* g2, const uint32_t* depth, const uint8_t* in, const void* pyramid,
                                uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t formatFlags, const uint32_t* params,
                                const uint32_t* gloss)
{
    using namespace cry;
    SsrParams p;
    SsrGlossParams gp;
    static_assert(sizeof p == 32 && sizeof gp == 16, "eight and four words");
    std::memcpy(&p, params, sizeof p);
    std::memcpy(&gp, gloss, sizeof gp);
    const SsrGlossLaunch L = ssr_gloss_launch(ssr_launch(proj, viewProj, invViewProj, eye, *nearZ, g0, g1, g2, depth, in, out, W, H, row0, rows, formatFlags, p),
                                              pyramid, gp);
    const SsrGlossArgs& a = L.args;
    const auto own = [](bool pred) { return pred; };
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t gy = g / a.s.tilesX, gx = g - gy * a.s.tilesX;
        for (uint32_t t = 0; t < kSsrThreads; ++t) {
            const uint32_t px = gx * kSsrGroupW + fog_lane_x(t), py = a.s.row0 + gy * kSsrTile + fog_lane_y(t);
            if (px >= a.s.W || py >= a.s.rowEnd) continue;
            ssr_pixel(a.s, px, py, own, SsrGlossHit{ a });
        }
    }
    return L.groups;
}
