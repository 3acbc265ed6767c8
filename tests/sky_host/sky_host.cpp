// sky_host.cpp -- csrc/sky_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan and constants (sky_launch) and the
// kernel's walk over a one-dimensional grid of workgroups, 256 threads each (an 8 x 8 texel tile per wavefront, four side by side), as
// sky_kernel does it; the wave vote is the lane's own predicate (the vote only skips work: sky_core.hpp).
#include <cstdint>
#include <cstring>
#include "sky_core.hpp"

// params: the 48 bytes of a crychic_sky_params.  Returns the number of workgroups walked.
extern "C" uint32_t skh_render_sky(uint8_t* cube, uint32_t dim, uint32_t face0, uint32_t faces, const void* params)
{
    using namespace cry;
    SkyParams p;
    std::memcpy(&p, params, sizeof p);
    const SkyLaunch L = sky_launch(cube, dim, face0, faces, p);
    const SkyArgs& a = L.args;
    const auto own = [](bool pred) { return pred; };
    for (uint32_t blk = 0; blk < L.groups; ++blk) {
        const uint32_t f = blk / a.groupsPerFace, g = blk - f * a.groupsPerFace;
        const uint32_t gy = g / a.tilesX, gx = g - gy * a.tilesX;
        for (uint32_t t = 0; t < kSkyThreads; ++t) {
            const uint32_t x = gx * kSkyGroupW + sky_lane_x(t), y = gy * kSkyTile + sky_lane_y(t);
            if (x >= a.dim || y >= a.dim) continue;
            const uint32_t face = a.face0 + f;
            a.cube[(face * a.dim + y) * a.dim + x] = sky_texel(a.k, face, x, y, a.rd, own);
        }
    }
    return L.groups;
}

extern "C" void skh_sun_colour(const void* params, float* rgb)
{
    cry::SkyParams p;
    std::memcpy(&p, params, sizeof p);
    cry::sky_sun_colour(p, rgb);
}
