// ssr_host.cpp -- csrc/ssr_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan and constants (ssr_launch) and the
// kernel's walk over a one-dimensional grid of workgroups, 256 threads each (an 8 x 8 pixel tile per wavefront, four side by side), as
// ssr_kernel does it; the wave vote is the lane's own predicate (the vote only skips work: ssr_core.hpp).
#include <cstdint>
#include <cstring>
#include "ssr_core.hpp"

// params: the eight words of crychic_ssr_params (tests/ssr_lib.py).  Returns the number of workgroups walked.
extern "C" uint32_t ssh_ssr(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, const float* nearZ, const void* g0,
                            const void* g1, const void* g2, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H,
                            uint32_t row0, uint32_t rows, uint32_t formatFlags, const uint32_t* params)
{
    using namespace cry;
    SsrParams p;
    static_assert(sizeof p == 32, "eight words");
    std::memcpy(&p, params, sizeof p);
    const SsrLaunch L = ssr_launch(proj, viewProj, invViewProj, eye, *nearZ, g0, g1, g2, depth, in, out, W, H, row0, rows, formatFlags, p);
    const SsrArgs& a = L.args;
    const auto own = [](bool pred) { return pred; };
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t gy = g / a.tilesX, gx = g - gy * a.tilesX;
        for (uint32_t t = 0; t < kSsrThreads; ++t) {
            const uint32_t px = gx * kSsrGroupW + fog_lane_x(t), py = a.row0 + gy * kSsrTile + fog_lane_y(t);
            if (px >= a.W || py >= a.rowEnd) continue;
            ssr_pixel(a, px, py, own);
        }
    }
    return L.groups;
}
