// fog_host.cpp -- csrc/fog_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan and constants (fog_launch) and the
// kernel's walk over a one-dimensional grid of workgroups, 256 threads each (an 8 x 8 pixel tile per wavefront, four side by side), as
// fog_kernel does it; the wave vote is the lane's own predicate (the vote only skips work: fog_core.hpp).
#include <cstdint>
#include <cstring>
#include "fog_core.hpp"

// params: { density bits, maxDistance bits, steps, ambient R G B, sun R G B } as nine uint32 (tests/fog_lib.py).  Returns the number
// of workgroups walked.
extern "C" uint32_t fgh_fog(const float* invViewProj, const float* eye, const float* shadowTransforms, const uint32_t* depth,
                            const uint32_t* const* maps, uint32_t dim, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                            uint32_t rows, const uint32_t* params)
{
    using namespace cry;
    FogParams p = {};
    std::memcpy(&p.density, &params[0], 4);
    std::memcpy(&p.maxDistance, &params[1], 4);
    p.steps = params[2];
    for (int k = 0; k < 3; ++k) { p.ambient[k] = (uint8_t)params[3 + k]; p.sun[k] = (uint8_t)params[6 + k]; }
    const FogLaunch L = fog_launch(invViewProj, eye, reinterpret_cast<const float (*)[16]>(shadowTransforms), depth, maps, dim, in, out, W, H,
                                   row0, rows, p);
    const FogArgs& a = L.args;
    const auto own = [](bool pred) { return pred; };
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t gy = g / a.tilesX, gx = g - gy * a.tilesX;
        for (uint32_t t = 0; t < kFogThreads; ++t) {
            const uint32_t px = gx * kFogGroupW + fog_lane_x(t), py = a.row0 + gy * kFogTile + fog_lane_y(t);
            if (px >= a.W || py >= a.rowEnd) continue;
            fog_pixel(a, px, py, own);
        }
    }
    return L.groups;
}
