// grade_core.hpp -- the body of crychic_grade (grade.hip) and the table builder behind
// crychic_grade_build_lut, written so that a host compiler builds them too (tests/grade_host): one call per thread and phase, the
// caller supplies the barrier between the two phases.  The definition is the comment in include/crychic_hip.h; this file restates
// none of it beyond what the code needs.
//
// Structure: a persistent launch.  Phase 1 (grade_stage): the workgroup copies the table's N^3 dwords into LDS.  Phase 2
// (grade_walk): the row range is one run of `count` consecutive texels; it is cut into a head of 0 .. 3 texels that brings `out` to a
// 16-byte boundary, a body of quads and a tail of 0 .. 3 texels.  The workgroups stride over the quads, 16 bytes per lane per load and
// store (VEC), or over single texels where `in` and `out` are not 16-byte aligned alike; the first lanes of workgroup 0 take the head
// and the tail.  A lane reads its texels before it writes them and no lane reads another's, so in == out is safe.
//
// Per texel: three (cell, fraction) pairs, four dword reads of the table, and the red and blue channels interpolated together in
// the two halves of one dword (each half stays below 65 536: the weights add up to 255, 255 * 255 + 127 = 65 152).  x / 255 is
// (x * 0x8081) >> 23, exact for every x below 65 536 (tests/grade_host counts the mismatches); the product stays below 2^32.
#pragma once
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kGradeMaxN = 33u;
constexpr uint32_t kGradeThreads = 1024u;
constexpr uint32_t kGradeLdsPerCu = 160u * 1024u;       // gfx950

struct GradeArgs {
    const uint32_t* in;         // the first texel of the row range
    uint32_t* out;
    const uint32_t* lut;
    uint32_t N, entries;        // entries = N^3
    uint32_t head, quads, tail; // VEC: head + 4 quads + tail texels; otherwise head = tail = 0 and `quads` counts single texels
};

typedef uint32_t GradeTexels4 __attribute__((ext_vector_type(4)));

CRY_HD uint32_t grade_div255(uint32_t x) { return (x * 0x8081u) >> 23; }       // x < 65 536

// (cell << 8) | fraction of one channel value; n1 = N - 1
CRY_HD uint32_t grade_cell(uint32_t v, uint32_t n1)
{
    const uint32_t p = mul24(v, n1);
    const uint32_t q = grade_div255(p);
    const uint32_t i = q < n1 - 1u ? q : n1 - 1u;
    return (i << 8) | (p - 255u * i);
}

// One texel through the table `lut` (LDS on the device).  Ties between fractions fall as the compares below let them: the vertex
// they decide has the weight 0.
CRY_HD uint32_t grade_texel(const uint32_t* lut, uint32_t N, uint32_t texel)
{
    const uint32_t n1 = N - 1u, NN = mul24(N, N);
    const uint32_t cr = grade_cell(texel & 255u, n1), cg = grade_cell((texel >> 8) & 255u, n1), cb = grade_cell((texel >> 16) & 255u, n1);
    const uint32_t fr = cr & 255u, fg = cg & 255u, fb = cb & 255u;
    const uint32_t v0 = (cr >> 8) + mul24(N, cg >> 8) + mul24(NN, cb >> 8);
    const uint32_t v3 = v0 + 1u + N + NN;
    const bool rTop = fr >= fg && fr >= fb, gTop = fg >= fb;
    const uint32_t f1 = rTop ? fr : (gTop ? fg : fb);
    const uint32_t s1 = rTop ? 1u : (gTop ? N : NN);
    const bool bLow = fb <= fr && fb <= fg, gLow = fg <= fr;
    const uint32_t f3 = bLow ? fb : (gLow ? fg : fr);
    const uint32_t s3 = bLow ? NN : (gLow ? N : 1u);
    const uint32_t f2 = fr + fg + fb - f1 - f3;
    const uint32_t l0 = lut[v0], l1 = lut[v0 + s1], l2 = lut[v3 - s3], l3 = lut[v3];
    const uint32_t w0 = 255u - f1, w1 = f1 - f2, w2 = f2 - f3;
    const uint32_t rb = mul24(w0, l0 & 0x00FF00FFu) + mul24(w1, l1 & 0x00FF00FFu) + mul24(w2, l2 & 0x00FF00FFu) + mul24(f3, l3 & 0x00FF00FFu) + 0x007F007Fu;
    const uint32_t g = mul24(w0, (l0 >> 8) & 255u) + mul24(w1, (l1 >> 8) & 255u) + mul24(w2, (l2 >> 8) & 255u) + mul24(f3, (l3 >> 8) & 255u) + 127u;
    return grade_div255(rb & 0xFFFFu) | (grade_div255(g) << 8) | (grade_div255(rb >> 16) << 16) | (texel & 0xFF000000u);
}

// Phase 1: thread t of `threads` copies its share of the table into `lds`.
CRY_HD void grade_stage(const GradeArgs& a, uint32_t t, uint32_t threads, uint32_t* lds)
{
    for (uint32_t i = t; i < a.entries; i += threads) lds[i] = a.lut[i];
}

// Phase 2: thread t of workgroup `group` of `groups`.
template <bool VEC>
CRY_HD void grade_walk(const GradeArgs& a, uint32_t group, uint32_t groups, uint32_t t, uint32_t threads, const uint32_t* lds)
{
    const uint32_t stride = groups * threads;       // the launcher keeps groups * threads far below 2^31
    if (VEC) {
        for (uint32_t q = group * threads + t; q < a.quads; q += stride) {
            const size_t at = (size_t)a.head + 4u * (size_t)q;
            GradeTexels4 v = *reinterpret_cast<const GradeTexels4*>(a.in + at);
            v[0] = grade_texel(lds, a.N, v[0]);
            v[1] = grade_texel(lds, a.N, v[1]);
            v[2] = grade_texel(lds, a.N, v[2]);
            v[3] = grade_texel(lds, a.N, v[3]);
            *reinterpret_cast<GradeTexels4*>(a.out + at) = v;
        }
        if (group == 0u && t < a.head + a.tail) {
            const size_t at = t < a.head ? t : (size_t)a.head + 4u * (size_t)a.quads + (t - a.head);
            a.out[at] = grade_texel(lds, a.N, a.in[at]);
        }
    } else {
        for (uint32_t q = group * threads + t; q < a.quads; q += stride) a.out[q] = grade_texel(lds, a.N, a.in[q]);
    }
}

// The launch plan (grade.hip's launcher and the host harness walk it): `cus` compute units.  One workgroup per compute unit at
// N = 33; two where two tables fit the LDS (1024 threads each: the 2048 a compute unit holds); never more workgroups than there is
// work for.
struct GradeLaunch { GradeArgs args; uint32_t groups, ldsBytes; bool vec; };
CRY_HD GradeLaunch grade_launch(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t row0, uint32_t rows, const uint8_t* lut, uint32_t N, uint32_t cus)
{
    GradeLaunch L;
    const size_t first = (size_t)row0 * W;
    const uint32_t count = rows * W;                // at most 2^28
    const uint8_t* src = in + 4u * first;
    uint8_t* dst = out + 4u * first;
    L.args.in = reinterpret_cast<const uint32_t*>(src);
    L.args.out = reinterpret_cast<uint32_t*>(dst);
    L.args.lut = reinterpret_cast<const uint32_t*>(lut);
    L.args.N = N;
    L.args.entries = N * N * N;
    L.ldsBytes = 4u * L.args.entries;
    L.vec = (((uintptr_t)src ^ (uintptr_t)dst) & 15u) == 0u;
    if (L.vec) {
        const uint32_t lead = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u) >> 2;
        L.args.head = lead < count ? lead : count;
        L.args.quads = (count - L.args.head) >> 2;
        L.args.tail = (count - L.args.head) & 3u;
    } else {
        L.args.head = L.args.tail = 0u;
        L.args.quads = count;
    }
    const uint32_t perCu = 2u * L.ldsBytes <= kGradeLdsPerCu ? 2u : 1u;
    const uint32_t want = (L.args.quads + kGradeThreads - 1u) / kGradeThreads;
    const uint32_t most = cus * perCu;
    L.groups = count == 0u ? 0u : (want < most ? (want ? want : 1u) : most);
    return L;
}

// ---- the table of an ASC CDL with a saturation (crychic_grade_build_lut; host code) ------------------------------------------------
struct GradeParams { float slope[3], offset[3], power[3], saturation; };

inline void grade_build_entry(const GradeParams& p, uint32_t N, const uint32_t idx[3], uint8_t* entry)
{
    float z[3];
    for (int c = 0; c < 3; ++c) {
        const float x = divf((float)idx[c], (float)(N - 1u));
        const float y = clampf(fma(x, p.slope[c], p.offset[c]), 0.0f, 1.0f);
        z[c] = p.power[c] == 1.0f ? y : det_pow(y, p.power[c]);
    }
    const float luma = fma(0.0722f, z[2], fma(0.7152f, z[1], 0.2126f * z[0]));
    for (int c = 0; c < 3; ++c) {
        const float w = p.saturation == 1.0f ? z[c] : fma(p.saturation, z[c] - luma, luma);
        entry[c] = (uint8_t)float_to_unorm8(w);
    }
    entry[3] = 255u;
}

inline void grade_build_lut(const GradeParams& p, uint32_t N, uint8_t* lut)
{
    for (uint32_t k = 0; k < N; ++k)
        for (uint32_t j = 0; j < N; ++j)
            for (uint32_t i = 0; i < N; ++i) {
                const uint32_t idx[3] = { i, j, k };
                grade_build_entry(p, N, idx, lut + 4u * ((size_t)i + N * ((size_t)j + N * (size_t)k)));
            }
}

}  // namespace cry
