// Host build of the sky shortcut's predicate (csrc/ssao_core.hpp), for tests/test_ssao_prologue_gpu.py: which wavefronts of an SSAO
// pass take the shortcut, which all-sky wavefronts are refused because geometry lies within reach, which are lit, and how many
// cells the largest rectangle of the frame has -- decided exactly as ssao_kernel and launch_ssao decide it, so that a test can
// assert on the CPU that its frames make the device run every path of the kernel's prologue.  TEST HARNESS ONLY.
#include <cstdint>
#include <vector>
#include "ssao_core.hpp"

using namespace cry;

extern "C" {

// out[0] wavefronts that take the shortcut, [1] all-sky wavefronts refused (geometry in reach, or cells the depth pass did not
// visit), [2] wavefronts with a lane that is not sky, [3] cells of the largest rectangle of an all-sky wavefront, [4] all-sky
// wavefronts whose rectangle has more cells than the wavefront has live lanes (the kernel's fallback loop), [5] those of them
// with more than 64 cells, [6] whether the constants enable the shortcut, [7] whether they enable the tap culling,
// [8] lanes for which ssao_sky_cell_of_lane() differs from the row-major division (must be 0).
void sp_classify(const crychic_ssao_constants* cb, const void* normal, const uint32_t* depth, uint32_t W, uint32_t H, uint32_t row0,
                 uint32_t rows, uint32_t* out)
{
    const uint32_t w2 = W / 2u, gpitch = geo_map_cols(W);
    for (int i = 0; i < 9; ++i) out[i] = 0u;
    // what launch_depth_pairs / launch_ssao prepare for these rows
    uint32_t c0, cn;
    depth_pass_cell_rows(H, row0, rows, &c0, &cn, -1);
    const bool limited = c0 > 0u || c0 + cn < zmin_map_rows(H);
    SkyReach sky = ssao_sky_reach(*cb, W, H);
    if (limited) {
        sky.y0 = 8 * (int)c0 - 2 < 0 ? 0 : 8 * (int)c0 - 2;
        sky.y1 = 8 * (int)(c0 + cn) - 2 > (int)H ? (int)H : 8 * (int)(c0 + cn) - 2;
    }
    out[6] = sky.enabled ? 1u : 0u;
    out[7] = ssao_cull_params(*cb).enabled ? 1u : 0u;
    // the geometry map as depth_pairs_kernel fills it: the texel rows its wavefronts visit, cell columns offset by -2 texels
    std::vector<uint8_t> geo((size_t)gpitch * geo_map_rows(H), 0);
    for (int ty = 8 * (int)c0 - 2; ty < 8 * (int)(c0 + cn) - 2; ++ty) {
        if ((uint32_t)ty >= H) continue;
        for (uint32_t tx = 0; tx < W; ++tx)
            if ((depth[(uint32_t)ty * W + tx] & 0x00FFFFFFu) != 0x00FFFFFFu) geo[((uint32_t)ty >> 5) * gpitch + (tx + 2u) / 128u] = 1;
    }
    const u2* nrm = (const u2*)normal;
    for (uint32_t y = row0; y < row0 + rows; ++y)
        for (uint32_t x0 = 0; x0 < w2; x0 += 64u) {
            const uint32_t n = (w2 - x0) < 64u ? (w2 - x0) : 64u;
            bool allSky = true;
            for (uint32_t k = 0; k < n; ++k) allSky = allSky && ssao_centre(*cb, nrm, depth, W, H, (int)(x0 + k), (int)y).sky;
            if (!allSky) { out[2]++; continue; }
            const GeoCells g = ssao_sky_cells(sky, W, H, x0, n, y);
            const uint32_t ncx = g.cx1 - g.cx0 + 1u, ncells = ncx * (g.cy1 - g.cy0 + 1u);
            bool geometry = false;
            for (uint32_t cy = g.cy0; cy <= g.cy1; ++cy)
                for (uint32_t cx = g.cx0; cx <= g.cx1; ++cx) geometry = geometry || geo[cy * gpitch + cx] != 0;
            if (sky.enabled && g.known && !geometry) out[0]++; else out[1]++;
            if (!sky.enabled) continue;
            out[3] = ncells > out[3] ? ncells : out[3];
            if (ncells > n) out[4]++;
            if (ncells > 64u) out[5]++;
            if (ncells <= 64u)
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const uint32_t k = lane < ncells ? lane : ncells - 1u;
                    if (ssao_sky_cell_of_lane(g, gpitch, lane) != (g.cy0 + k / ncx) * gpitch + g.cx0 + k % ncx) out[8]++;
                }
        }
}

// ssao_sky_cell_of_lane() against the division for every rectangle of at most 64 cells and every lane; returns the mismatches
uint32_t sp_cell_of_lane_mismatches(void)
{
    uint32_t bad = 0;
    for (uint32_t ncx = 1; ncx <= 64u; ++ncx)
        for (uint32_t ncy = 1; ncx * ncy <= 64u; ++ncy)
            for (uint32_t pitch = ncx; pitch <= ncx + 70u; pitch += 7u) {
                const GeoCells g{ 3u, 3u + ncx - 1u, 5u, 5u + ncy - 1u, true };
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const uint32_t k = lane < ncx * ncy ? lane : ncx * ncy - 1u;
                    if (ssao_sky_cell_of_lane(g, pitch + 3u, lane) != (5u + k / ncx) * (pitch + 3u) + 3u + k % ncx) bad++;
                }
            }
    return bad;
}

}
