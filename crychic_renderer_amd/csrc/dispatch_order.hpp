// dispatch_order.hpp -- the order in which the SSAO and lighting launches meet the bands of the frame (DESIGN.md section 4
// "Dispatch order over time").  Host and device: tests/test_dispatch_order.py builds the map with the host compiler.
//
// Workgroups are dispatched in increasing blockIdx order, so with the natural mapping a launch walks the frame top to bottom: on a
// frame with sky above ground it first streams the cheap bands and then runs the costly ones, and drains on the costliest.  The map
// below deals the bands of `ways` distant segments of the frame in turn, so that cheap and costly bands are in flight together
// whatever the frame holds.  Placement is a performance hint only: any dispatch order produces the same pixels.
#pragma once
#include <stdint.h>

#if !defined(CRY_HD)                // devmath.hpp's definition; this header stands alone so that any host compiler builds it
#if defined(__HIPCC__)
#define CRY_HD __host__ __device__ __forceinline__
#else
#define CRY_HD inline
#endif
#endif

// Segments per kernel family.  1 = natural order, 0 = plain reversal (bottom-up), n >= 2 = n interleaved segments.  Compile-time
// constants; probe builds override them with -D (tools/probes/variants.sh).  The defaults are the measured ones of
// profiles/dispatch_order_ab.txt (4K benchmark frame, per-kernel times in us): no interleave beat the natural order for either
// kernel (lighting 72.4 natural, 73.0 two ways, 75.4 four ways, 77.0 reversed; SSAO 55.6 natural, 56.6 two, 56.8 four), so the
// lighting kernels keep the natural order, and the SSAO pass takes the reversal (51.6): its costly wavefronts are the VALU-bound
// ones over geometry, and a launch that ends on the short sky wavefronts drains faster than one that ends on the costly ones.
// The reversal is NOT content-agnostic: it assumes what nearly every outdoor frame shows, sky above ground.  A frame with the sky
// below would lose what this one gains; a frame without sky moves by under one per cent either way (the covered camera: +0.8 us).
#ifndef CRY_LIGHT_BAND_WAYS
#define CRY_LIGHT_BAND_WAYS 1
#endif
#ifndef CRY_SSAO_BAND_WAYS
#define CRY_SSAO_BAND_WAYS 0
#endif

namespace cry {

// The band of the frame that the k-th band of the dispatch order covers: a bijection of [0, nBands) for every nBands >= 1.
// The frame's bands are cut into `ways` contiguous segments, the first nBands % ways of them one band longer than the others;
// dispatch takes the next band of segment 0, of segment 1, ... of segment ways - 1, and round again; the last bands of the longer
// segments follow in their natural order.  `ways` is a constant at every call site, so the two divisions below are by constants.
CRY_HD uint32_t band_of(uint32_t k, uint32_t nBands, uint32_t ways)
{
    if (ways == 0u) return nBands - 1u - k;
    if (ways == 1u) return k;
    const uint32_t q = nBands / ways, r = nBands - q * ways;       // segment s: q + (s < r) bands from s * q + min(s, r)
    const uint32_t i = k / ways, s = k - i * ways;
    if (i < q) return s * q + (s < r ? s : r) + i;
    const uint32_t j = k - q * ways;                               // the q-th band of segment j < r
    return j * q + j + q;
}

// band_of for a launch: one with fewer than 2 * ways bands (a small frame, a strip of a multi-GPU frame) keeps the natural order;
// the reversal counts as two segments here (the top and the bottom half change places).
CRY_HD uint32_t launch_band(uint32_t k, uint32_t nBands, uint32_t ways)
{
    return nBands < 2u * (ways < 2u ? 2u : ways) ? k : band_of(k, nBands, ways);
}

// Lighting: a band is kLightBandRows consecutive tile rows (32 pixel rows), so the ambient, cube and cascade lines that vertically
// adjacent tile rows share stay together in L2.  The tile rows past the last whole band keep their place at the end.
constexpr uint32_t kLightBandRows = 8u;
CRY_HD uint32_t light_dispatch_row(uint32_t by, uint32_t tileRows)
{
    const uint32_t nBands = tileRows / kLightBandRows;
    if (by >= nBands * kLightBandRows) return by;
    return launch_band(by / kLightBandRows, nBands, CRY_LIGHT_BAND_WAYS) * kLightBandRows + by % kLightBandRows;
}

}  // namespace cry
