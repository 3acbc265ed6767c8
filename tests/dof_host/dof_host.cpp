// dof_host.cpp -- csrc/dof_core.hpp built for the host (TEST INFRASTRUCTURE): the launcher's plan and constants (dof_launch) and the
// kernel's walk over a one-dimensional grid of workgroups, 256 threads each, as dof_kernel does it: the LDS window is one array kept
// across the workgroups (what a workgroup does not stage it must not read), the loop over the threads of a phase stands for the
// barrier behind it, and the reduction of the wavefronts' largest circle of confusion is a plain maximum.
#include <cstdint>
#include <cstring>
#include <vector>
#include "dof_core.hpp"

// params: { focusDistance bits, aperture bits, maxRadius } as three uint32 (tests/dof_host_lib.py); proj: 16 floats, the pass
// constants' Proj.  Returns the number of workgroups walked.
extern "C" uint32_t dfh_dof(const float* proj, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                            uint32_t rows, const uint32_t* params)
{
    using namespace cry;
    DofParams p = {};
    std::memcpy(&p.focusDistance, &params[0], 4);
    std::memcpy(&p.aperture, &params[1], 4);
    p.maxRadius = params[2];
    const DofLaunch L = dof_launch(proj, depth, in, out, W, H, row0, rows, p);
    const DofArgs& a = L.args;
    std::vector<DofTexel> lds(kDofLdsTexels, DofTexel{ 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu });
    for (uint32_t g = 0; g < L.groups; ++g) {
        const uint32_t tileY = g / a.tilesX, tileX = g - tileY * a.tilesX;
        uint32_t cmax = 0u;
        for (uint32_t t = 0; t < kDofThreads; ++t) {
            const uint32_t m = dof_stage(a, tileX, tileY, t, lds.data());
            cmax = m > cmax ? m : cmax;
        }
        for (uint32_t t = 0; t < kDofThreads; ++t) dof_gather(a, tileX, tileY, t, lds.data(), cmax);      // behind the barrier
    }
    return L.groups;
}

// The tap table as the kernel walks it: entry i of 197 (and the sentinel, i = 197), and the disc sizes count[0 .. 8].
extern "C" uint32_t dfh_tap(uint32_t i) { return cry::kDofTaps.e[i]; }
extern "C" uint32_t dfh_disc(uint32_t R) { return cry::kDofTaps.count[R]; }
