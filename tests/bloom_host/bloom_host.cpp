// bloom_host.cpp -- csrc/bloom_core.hpp built for the host (TEST INFRASTRUCTURE): the launch plans (bloom_plan, bloom_down_launch,
// bloom_unwind_args, bloom_composite_launch) and the kernels' walks as bloom.hip does them.  The LDS arrays are kept across the
// workgroups and start as 0xDEADBEEF (what a workgroup does not stage it must not read), the loop over the threads of a phase stands
// for the barrier behind it, the downsample's vote is an OR over the workgroup, and the composite's vote is taken over each run of 64
// threads.
#include <cstdint>
#include <cstring>
#include <vector>
#include "bloom_core.hpp"

namespace {
using namespace cry;

struct Lds {
    std::vector<BloomTexel> win;
    std::vector<uint32_t> sums;
    Lds() : win(kBloomWinTexels, BloomTexel{ 0xDEADBEEFu, 0xDEADBEEFu }), sums(kBloomRowSums, 0xDEADBEEFu) {}
};

template <bool First>
uint32_t run_down(const BloomDownLaunch& L, Lds& lds, uint32_t* zeroTiles)
{
    const BloomDownArgs& a = L.args;
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t tileY = g / a.tilesX, tileX = g - tileY * a.tilesX;
        uint32_t any = 0u;
        for (uint32_t t = 0; t < kBloomThreads; ++t) any |= bloom_down_stage<First>(a, tileX, tileY, t, lds.win.data());
        if (!any) {
            for (uint32_t t = 0; t < kBloomThreads; ++t) bloom_down_zero(a, tileX, tileY, t);
            ++*zeroTiles;
            continue;
        }
        for (uint32_t t = 0; t < kBloomThreads; ++t) bloom_down_rows(t, lds.win.data(), lds.sums.data());
        for (uint32_t t = 0; t < kBloomThreads; ++t) bloom_down_columns(a, tileX, tileY, t, lds.sums.data());
    }
    return L.groups;
}

void run_pyramid(const uint8_t* in, uint32_t W, uint32_t H, const BloomParams& p, uint8_t* ws, uint32_t* stats)
{
    const BloomPlan plan = bloom_plan(W, H, p.levels);
    Lds lds;
    for (uint32_t k = 1; k <= plan.nEff; ++k) {
        if (k == 1u) stats[0] += run_down<true>(bloom_down_launch(in, ws + plan.off[1], W, H, &p), lds, &stats[1]);
        else stats[0] += run_down<false>(bloom_down_launch(ws + plan.off[k - 1u], ws + plan.off[k], plan.w[k - 1u], plan.h[k - 1u], nullptr), lds, &stats[1]);
    }
    for (uint32_t k = plan.nEff - 1u; k >= 1u; --k) {
        const BloomUnwindArgs a = bloom_unwind_args(ws + plan.off[k], ws + plan.off[k + 1u], plan.w[k], plan.h[k], p.scatter);
        const uint32_t groups = (a.n + kBloomThreads - 1u) / kBloomThreads;
        for (uint32_t i = 0; i < groups * kBloomThreads; ++i) bloom_unwind(a, i);
        stats[0] += groups;
    }
}

void run_composite(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const BloomParams& p, const uint8_t* ws,
                   uint32_t* stats)
{
    const BloomPlan plan = bloom_plan(W, H, p.levels);
    const BloomCompositeLaunch L = bloom_composite_launch(in, out, ws + plan.off[1], W, H, row0, rows, p.intensity);
    BloomCompositeLane lanes[64];
    for (uint32_t w = 0; w < L.groups * kBloomWaves; ++w) {
        uint32_t added = 0u;
        for (uint32_t l = 0; l < 64u; ++l) {
            lanes[l] = bloom_composite_eval(L.args, w * 64u + l);
            added |= lanes[l].added;
        }
        if (L.args.inPlace && !added) { ++stats[2]; continue; }
        for (uint32_t l = 0; l < 64u; ++l) bloom_composite_store(L.args, lanes[l]);
    }
    stats[0] += L.groups;
    stats[3] += L.args.vec;
}
}  // namespace

// params: { threshold, knee, scatter, intensity, levels }; what: bit 0 the pyramid, bit 1 the composite of rows [row0, row0 + rows).
// stats (4 words, added to): workgroups walked, downsample tiles stored as zeros, composite wavefronts that stored nothing, composite
// launches that took the 16-byte path.
extern "C" void bh_bloom(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint32_t* params, uint8_t* workspace,
                         uint32_t what, uint32_t* stats)
{
    BloomParams p = {};
    p.threshold = params[0]; p.knee = params[1]; p.scatter = params[2]; p.intensity = params[3]; p.levels = params[4];
    if (what & 1u) run_pyramid(in, W, H, p, workspace, stats);
    if (what & 2u) run_composite(in, out, W, H, row0, rows, p, workspace, stats);
}

// The weight by the kernel's multiply-high against the definition's division, over every luma and threshold difference and every
// knee: the number of (n, K) pairs that differ.
extern "C" uint32_t bh_weight_mismatches()
{
    uint32_t bad = 0u;
    for (uint32_t K = 1; K <= 255u; ++K) {
        const uint32_t magic = (1u << 24) / K + 1u;
        for (uint32_t n = 1; n <= 65280u; ++n) {
            const uint32_t q = n / K, want = q < 256u ? q : 256u;
            bad += cry::bloom_weight(n, 0u, magic) != want;
        }
    }
    return bad;
}

extern "C" size_t bh_workspace_bytes(uint32_t W, uint32_t H, uint32_t levels) { return cry::bloom_plan(W, H, levels).bytes; }
