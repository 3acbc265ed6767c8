// Host harness of the split replay body (csrc/blur_tiles.hpp blur_replay_fetch_masks / _rows / _cols; TEST HARNESS ONLY): the
// blur chain the way api.cpp issues it, like hostsim.cpp's hs_blur_chain, with the replayed iterations through either
// blur_replay_tile (body 0) or blur_replay_tile_split (body 1), one sequential "thread" per tile, and the settle predicate of the
// pair launch per tile for the tests that have to know which tiles of a pair settle.
#include <cstdint>
#include <vector>

#include "blur_tiles.hpp"

using namespace cry;

extern "C" {

// planes[blur_chain_ssao_plane(blurCount)] holds the SSAO output for rows blur_chain_ssao_rows(..), written with `stamp` (the
// unoccluded-wavefront map of the workspace belongs to it); the result is in plane0, rows [row0, row0 + rows).
// body: 0 = blur_replay_tile, 1 = blur_replay_tile_split.  poison != 0: around every replayed tile the decision words of its ten
// apron columns (x0 - 5 .. x0 - 1 and x0 + 64 .. x0 + 68, CLAMPed as the staging clamps them, every staged row) hold `poison`
// while the tile runs and their recorded values again afterwards -- except where a clamped apron column IS one of the tile's own
// columns (x0 = 0, or the last column of a ragged width), which the tile does read.
// settled: one byte per tile of the 64 x 16 grid, 1 = the pair launch settled it (blurCount > 1 only); may be null.
void bm_blur_chain(const crychic_ssao_constants* cb, void* edge_base, uint16_t* plane0, uint16_t* plane1, uint32_t W, uint32_t H, int blurCount,
                   uint32_t row0, uint32_t rows, uint32_t stamp, int onesMargin, int body, uint32_t poison, uint8_t* settled)
{
    const uint32_t h2 = H / 2, w2 = W / 2;
    const EdgePlane e = edge_plane_carve(edge_base, W, H);
    uint16_t* planes[2] = { plane0, plane1 };
    uint32_t sr0, srn;
    blur_chain_ssao_rows(blurCount, row0, rows, h2, &sr0, &srn);
    const bool positive = blur_weights_positive(*cb);        // as the launchers decide
    if (!positive) stamp = 0u;
    std::vector<f4a> s_nz(kBlurPairSW * kBlurPairSH);
    std::vector<float> s_a(kBlurPairSW * kBlurPairSH), s_mid(kBlurTileW * kBlurPairSH);
    std::vector<uint32_t> s_mask(kBlurPairSW * kBlurPairSH), s_rows(kBlurMaxWaves);
    std::vector<uint16_t> s_hmask(kBlurTileW * kBlurTileH);
    std::vector<uint32_t> saved;
    for (int i = 0; i < blur_chain_launches(blurCount); ++i) {
        const BlurStep st = blur_chain_step(blurCount, row0, rows, h2, i);
        if (st.rows == 0) continue;
        const uint32_t t0 = st.row0 / (uint32_t)kBlurTileH, t1 = (st.row0 + st.rows - 1u) / (uint32_t)kBlurTileH;
        for (uint32_t ty = t0; ty <= t1; ++ty)
            for (uint32_t tx = 0; tx < blur_tiles_x(W); ++tx) {
                BlurTileArgs a;
                a.w = &cb->BlurWeights[0][0]; a.e = e; a.in = planes[st.in]; a.out = planes[st.out];
                a.w2 = (int)w2; a.h2 = (int)h2; a.x0 = (int)tx * kBlurTileW; a.y0 = (int)ty * kBlurTileH;
                a.row0 = (int)st.row0; a.row1 = (int)(st.row0 + st.rows);
                a.borderZ = ndc_to_view(*cb, 1.0f);
                a.tileIndex = ty * blur_tiles_x(W) + tx;
                if (i == 0) {
                    if (blurCount > 1) blur_pair_tile<true>(BlockSeq{}, a, stamp, onesMargin, (int)sr0, (int)(sr0 + srn), s_nz.data(), s_a.data(), s_mid.data(), s_hmask.data());
                    else blur_pair_tile<false>(BlockSeq{}, a, stamp, onesMargin, (int)sr0, (int)(sr0 + srn), s_nz.data(), s_a.data(), s_mid.data(), s_hmask.data());
                    if (settled && blurCount > 1) settled[a.tileIndex] = stamp != 0u && e.tiles[a.tileIndex] == stamp ? 1 : 0;
                    continue;
                }
                // the apron columns' words, CLAMPed as the staging clamps them
                std::vector<uint32_t> where;
                if (poison != 0u) {
                    const int x1 = a.x0 + kBlurTileW < a.w2 ? a.x0 + kBlurTileW : a.w2;        // one past the tile's own last column
                    for (int ly = 0; ly < kBlurPairSH; ++ly) {
                        const int cy = clampi(a.y0 - kBlurRadius + ly, 0, a.h2 - 1);
                        for (int k = 0; k < 2 * kBlurRadius; ++k) {
                            const int cx = clampi(k < kBlurRadius ? a.x0 - kBlurRadius + k : a.x0 + kBlurTileW + k - kBlurRadius, 0, a.w2 - 1);
                            if (cx >= a.x0 && cx < x1) continue;
                            where.push_back((uint32_t)cy * w2 + (uint32_t)cx);
                        }
                    }
                    saved.resize(where.size());
                    for (size_t k = 0; k < where.size(); ++k) saved[k] = e.masks[where[k]];
                    for (size_t k = 0; k < where.size(); ++k) e.masks[where[k]] = poison;
                }
                if (body == 0) blur_replay_tile(BlockSeq{}, a, stamp, positive, s_a.data(), s_mask.data(), s_mid.data(), s_rows.data());
                else blur_replay_tile_split<1>(BlockSeq{}, a, stamp, positive, s_a.data(), s_mid.data(), s_rows.data());
                for (size_t k = where.size(); k-- > 0;) e.masks[where[k]] = saved[k];
            }
    }
}

}  // extern "C"
