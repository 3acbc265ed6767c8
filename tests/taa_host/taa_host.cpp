// taa_host.cpp -- csrc/taa_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan and constants (taa_launch) and the
// kernel's walk over a one-dimensional grid of workgroups, 256 threads each (an 8 x 8 pixel tile per wavefront, four side by side), as
// taa_kernel does it; the wave vote is the lane's own predicate (the vote only skips work: taa_core.hpp).
#include <cstdint>
#include "taa_core.hpp"

// Returns the number of workgroups walked.
extern "C" uint32_t tah_taa(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, const uint8_t* in,
                            const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                            uint32_t blend, uint32_t flags)
{
    using namespace cry;
    TaaParams p = {};
    p.blend = blend;
    p.flags = flags;
    const TaaLaunch L = taa_launch(invViewProj, curViewProj, prevViewProj, depth, in, historyIn, historyOut, out, W, H, row0, rows, p);
    const TaaArgs& a = L.args;
    const auto own = [](bool pred) { return pred; };
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t gy = g / a.tilesX, gx = g - gy * a.tilesX;
        for (uint32_t t = 0; t < kTaaThreads; ++t) {
            const uint32_t px = gx * kTaaGroupW + taa_lane_x(t), py = a.row0 + gy * kTaaTile + taa_lane_y(t);
            if (px >= a.W || py >= a.rowEnd) continue;
            taa_pixel(a, px, py, own);
        }
    }
    return L.groups;
}

// the tile's sides, for the tests' frame sizes
extern "C" void tah_tile(uint32_t* groupW, uint32_t* groupH) { *groupW = cry::kTaaGroupW; *groupH = cry::kTaaTile; }
