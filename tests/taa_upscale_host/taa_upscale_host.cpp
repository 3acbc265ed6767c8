// taa_upscale_host.cpp -- csrc/taa_upscale_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan and constants
// (taa_upscale_launch) and the kernel's walk over a one-dimensional grid of workgroups, 256 threads each (an 8 x 8 output tile per
// wavefront, four side by side), as taa_upscale_kernel does it; the wave vote is the lane's own predicate (the vote only skips work).
#include <cstdint>
#include "taa_upscale_core.hpp"

// Returns the number of workgroups walked.
extern "C" uint32_t tuh_taa_upscale(const float* invViewProj, const float* curViewProj, const float* prevViewProj, float jx, float jy, const uint32_t* depth,
                                    const uint8_t* in, uint32_t Wi, uint32_t Hi, const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out,
                                    uint32_t Wo, uint32_t Ho, uint32_t row0, uint32_t rows, uint32_t blend, uint32_t flags)
{
    using namespace cry;
    TaaUpscaleParams p = {};
    p.blend = blend;
    p.flags = flags;
    const TaaUpscaleLaunch L = taa_upscale_launch(invViewProj, curViewProj, prevViewProj, jx, jy, depth, in, Wi, Hi, historyIn, historyOut, out, Wo, Ho,
                                                  row0, rows, p);
    const TaaUpscaleArgs& a = L.args;
    const auto own = [](bool pred) { return pred; };
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t gy = g / a.tilesX, gx = g - gy * a.tilesX;
        for (uint32_t t = 0; t < kTaaThreads; ++t) {
            const uint32_t ox = gx * kTaaGroupW + taa_lane_x(t), oy = a.row0 + gy * kTaaTile + taa_lane_y(t);
            if (ox >= a.Wo || oy >= a.rowEnd) continue;
            taa_upscale_pixel(a, ox, oy, own);
        }
    }
    return L.groups;
}

// the position of step 1 on either path whatever the sizes (the 64-bit path is what frames of more than 2^24 Ni No take), and the
// division by a divisor known on the host
extern "C" int32_t tuh_position(uint32_t o, uint32_t Ni, uint32_t No, int32_t J, int narrow)
{
    return cry::tu_position(o, Ni, No, cry::tu_magic(No), J, narrow != 0);
}
extern "C" uint32_t tuh_div(uint32_t n, uint32_t d) { return cry::tu_div(n, d, cry::tu_magic(d)); }
