// post_aa_host.cpp -- csrc/post_aa_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan (post_aa_launch) and the
// kernel's three phases over a grid of 64 x 32 tiles, 256 threads per tile; the loop over the threads of a phase stands for the
// workgroup barrier behind it, and the wave vote is the lane's own predicate (the vote only skips work: post_aa_core.hpp).
#include <cstdint>
#include <memory>
#include <vector>
#include "post_aa_core.hpp"

// path: 0 = what the launcher would choose, 1 = the 16-byte path (refused, -1, where the launcher could not choose it), 2 = the
// dword path.  Returns the path taken (1 or 2).
extern "C" int pah_antialias(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint32_t* params,
                             int path)
{
    using namespace cry;
    const PostAaParams p = { params[0], params[1], params[2], params[3] };
    const PostAaLaunch L = post_aa_launch(in, out, W, H, row0, rows, p);
    if (path == 1 && !L.vec) return -1;
    const bool vec = path == 0 ? L.vec : path == 1;
    std::vector<uint16_t> tile(kAaLdsTexels + 4u);
    uint16_t* lds = tile.data();
    while (reinterpret_cast<uintptr_t>(lds) & 7u) ++lds;                // the kernel's array is 16-byte aligned; the body needs 8
    std::vector<PostAaLane> lanes(kAaThreads);
    std::unique_ptr<PostAaEdgeList> edges(new PostAaEdgeList);
    const auto own = [](bool pred) { return pred; };
    for (uint32_t ty = 0; ty < L.tilesY; ++ty)
        for (uint32_t tx = 0; tx < L.tilesX; ++tx) {
            edges->count = 0u;
            for (uint32_t t = 0; t < kAaThreads; ++t) {
                if (vec) post_aa_fill<true>(L.args, tx, ty, t, lds, lanes[t]);
                else post_aa_fill<false>(L.args, tx, ty, t, lds, lanes[t]);
            }
            for (uint32_t t = 0; t < kAaThreads; ++t) {                 // behind the barrier
                if (vec) post_aa_detect<true>(L.args, tx, ty, t, lds, lanes[t], edges.get());
                else post_aa_detect<false>(L.args, tx, ty, t, lds, lanes[t], edges.get());
            }
            for (uint32_t t = 0; t < kAaThreads; ++t) post_aa_edges(L.args, tx, ty, t, lds, edges.get(), own);      // behind the second
        }
    return vec ? 1 : 2;
}
