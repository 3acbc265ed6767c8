// cube_mips_host.cpp -- csrc/cube_mips_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan (cube_mips_launch) and
// the kernel's per-phase bodies (cube_mips_tile_phase_first / _next, which cube_mips_tile calls between barriers), a grid of 64 x 64 tiles per face,
// 256 threads per tile; the loop over the threads of a phase stands for the workgroup barrier behind it.
#include <cstdint>
#include <vector>
#include "cube_mips_core.hpp"

extern "C" void cmh_generate(uint8_t* chain, uint32_t dim, uint32_t levels)
{
    using namespace cry;
    std::vector<uint32_t> tile(kCubeMipTileWords);
    for (uint32_t i = 0; i < cube_mips_launches(levels); ++i) {
        const CubeMipLaunch L = cube_mips_launch(chain, dim, levels, i);
        for (uint32_t face = 0; face < 6u; ++face)
            for (uint32_t ty = 0; ty < L.tiles; ++ty)
                for (uint32_t tx = 0; tx < L.tiles; ++tx)
                    for (uint32_t j = 1u; j <= L.nLevels; ++j)               // a phase for all threads, then the next: the barrier
                        for (uint32_t t = 0; t < kCubeMipThreads; ++t) {
                            if (j > 1u) cube_mips_tile_phase_next(L.levelIn, L.dIn, j, face, tx, ty, t, tile.data());
                            else if (L.vec) cube_mips_tile_phase_first<true>(L.levelIn, L.dIn, face, tx, ty, t, tile.data());
                            else cube_mips_tile_phase_first<false>(L.levelIn, L.dIn, face, tx, ty, t, tile.data());
                        }
    }
}
