// grade_host.cpp -- csrc/grade_core.hpp built for the host (TEST INFRASTRUCTURE): the launch plan and the kernel's two phases as
// grade.hip runs them.  The LDS array is exactly 4 N^3 bytes and starts every workgroup as 0xDEADBEEF (what a workgroup does not stage
// it must not read), and the loop over the threads of a phase stands for the barrier behind it.
#include <cstdint>
#include <cstring>
#include <vector>
#include "grade_core.hpp"

// stats (2 words, added to): workgroups walked, launches that took the 16-byte path.  `cus`: the compute units the plan is made for.
extern "C" void gh_grade(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint8_t* lut, uint32_t N,
                         uint32_t cus, uint32_t* stats)
{
    using namespace cry;
    (void)H;
    if (rows == 0u) return;
    const GradeLaunch L = grade_launch(in, out, W, row0, rows, lut, N, cus);
    for (uint32_t g = 0; g < L.groups; ++g) {
        std::vector<uint32_t> lds(L.ldsBytes / 4u, 0xDEADBEEFu);
        for (uint32_t t = 0; t < kGradeThreads; ++t) grade_stage(L.args, t, kGradeThreads, lds.data());
        for (uint32_t t = 0; t < kGradeThreads; ++t) {
            if (L.vec) grade_walk<true>(L.args, g, L.groups, t, kGradeThreads, lds.data());
            else grade_walk<false>(L.args, g, L.groups, t, kGradeThreads, lds.data());
        }
    }
    if (stats) { stats[0] += L.groups; stats[1] += L.vec ? 1u : 0u; }
}

// The kernel's x / 255 against the division, over every x below 65 536: the number that differ.
extern "C" uint32_t gh_div255_mismatches()
{
    uint32_t bad = 0u;
    for (uint32_t x = 0; x < 65536u; ++x) bad += cry::grade_div255(x) != x / 255u;
    return bad;
}

// params: slope[3], offset[3], power[3], saturation -- unchecked, as crychic_grade_build_lut hands them on
extern "C" void gh_build_lut(const float* params, uint32_t N, uint8_t* lut)
{
    cry::GradeParams p;
    std::memcpy(&p, params, sizeof p);
    cry::grade_build_lut(p, N, lut);
}
