// sharpen_host.cpp -- csrc/sharpen_core.hpp built for the host (TEST INFRASTRUCTURE): the launch plan and the kernels' bodies as
// sharpen.hip runs them.  A wavefront of the wide kernel is 64 lanes in lockstep: every lane loads its row, then the exchange goes
// through two arrays (what the kernel does with two lane permutes), then every lane computes and stores.  A lane's left and right
// start as 0xDEADBEEF where the exchange has to fill them, so a pixel that it does not deliver shows.
#include <cstdint>
#include <cstring>
#include "sharpen_core.hpp"

namespace {
using namespace cry;

struct Wave { SharpenLane lane[kSharpenWave]; };

void wave_row(const SharpenArgs& a, const Wave& w, uint32_t y, SharpenRow* rows)
{
    uint32_t up[kSharpenWave], down[kSharpenWave];
    for (uint32_t l = 0; l < kSharpenWave; ++l) {
        rows[l] = sharpen_load_row(a, w.lane[l], y);
        if (l != 0u && l != kSharpenWave - 1u) rows[l].left = rows[l].right = 0xDEADBEEFu;
        up[l] = sharpen_exchange_up(rows[l]);
        down[l] = sharpen_exchange_down(rows[l]);
    }
    for (uint32_t l = 0; l < kSharpenWave; ++l)
        sharpen_exchange_take(w.lane[l], rows[l], up[(l + kSharpenWave - 1u) % kSharpenWave], down[(l + 1u) % kSharpenWave]);
}

void wide_wave(const SharpenArgs& a, uint32_t group, uint32_t firstThread)
{
    if (sharpen_wave_idle(a, group, firstThread)) return;
    Wave w;
    for (uint32_t l = 0; l < kSharpenWave; ++l) w.lane[l] = sharpen_lane(a, group, firstThread + l);
    SharpenPx4 up[kSharpenWave];
    SharpenRow mid[kSharpenWave], dn[kSharpenWave];
    const uint32_t y0 = w.lane[0].y0, y1 = w.lane[0].y1;
    for (uint32_t l = 0; l < kSharpenWave; ++l) up[l] = sharpen_load_row(a, w.lane[l], sharpen_row_above(y0)).px;
    wave_row(a, w, y0, mid);
    for (uint32_t y = y0; y < y1; ++y) {
        wave_row(a, w, sharpen_row_below(a, y), dn);
        for (uint32_t l = 0; l < kSharpenWave; ++l) {
            sharpen_store(a, w.lane[l], y, sharpen_quad(a, up[l], mid[l], dn[l].px));
            up[l] = mid[l].px;
            mid[l] = dn[l];
        }
    }
}
}  // namespace

// stats (2 words, added to): workgroups walked, launches that took the wide path
extern "C" void sh_sharpen(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t strength, uint32_t limit,
                           uint32_t* stats)
{
    if (rows == 0u) return;
    const SharpenLaunch L = sharpen_launch(in, out, W, H, row0, rows, strength, limit);
    for (uint32_t g = 0; g < L.groups; ++g) {
        if (L.wide) {
            for (uint32_t t = 0; t < kSharpenThreads; t += kSharpenWave) wide_wave(L.args, g, t);
        } else {
            for (uint32_t t = 0; t < kSharpenThreads; ++t)
                if (g * kSharpenThreads + t < rows * W) sharpen_narrow(L.args, g * kSharpenThreads + t);
        }
    }
    if (stats) { stats[0] += L.groups; stats[1] += L.wide ? 1u : 0u; }
}

static float nudge(float r, int ulps)
{
    uint32_t u;
    std::memcpy(&u, &r, 4);
    u += (uint32_t)ulps;            // r is positive and normal: the neighbouring binary32 values
    std::memcpy(&r, &u, 4);
    return r;
}

// sharpen_q12 of the ratio against (n << 12) / d over every n <= d, 1 <= d <= 255, the reciprocal moved by `ulps` units in the last
// place: the number that differ.  The pairs a pixel can produce are mn / mx and (255 - mx) / (255 - mn), mn <= mx: exactly these.
extern "C" uint32_t sh_q12_mismatches(int ulps)
{
    uint32_t bad = 0u;
    for (uint32_t d = 1; d <= 255u; ++d) {
        const float r = nudge(cry::sharpen_rcp((float)d), ulps);
        for (uint32_t n = 0; n <= d; ++n) bad += cry::sharpen_q12((float)n * r) != (n << 12) / d;
    }
    return bad;
}

// sharpen_div as sharpen_pixel calls it against the definition's (num + den / 2) / den, den = 4 (4096 - t), over every num < 2^22
// and every t in [t0, t1): the number that differ.  The routine sees num only through (num + den / 2) >> 2: each of its values is
// tried once and stands for the four numerators that share it (floor(x / 4 D) = floor((x >> 2) / D) is a theorem; every 4099th
// numerator and its three successors try it all the same).
extern "C" uint64_t sh_div_mismatches(uint32_t t0, uint32_t t1, int ulps)
{
    uint64_t bad = 0u;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t D = 4096u - t, den = 4u * D;
        const float r = nudge(cry::sharpen_rcp((float)D), ulps);
        const uint32_t first = (den / 2u) >> 2, last = ((1u << 22) - 1u + den / 2u) >> 2;
        uint32_t wrong = 0u;
        for (uint32_t n = first; n <= last; ++n) {
            const uint32_t q = cry::sharpen_div(n, r);
            wrong += (q * D > n) | (n - q * D >= D);            // q is not floor(n / D)
        }
        bad += wrong;
        for (uint32_t num = 0; num < (1u << 22); num += 4099u)                         // floor(x / (4 D)) == floor((x >> 2) / D)
            for (uint32_t k = 0; k < 4u; ++k) bad += (num + k + den / 2u) / den != ((num + k + den / 2u) >> 2) / D;
    }
    return bad;
}
