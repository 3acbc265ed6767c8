// ssao_guards_san_main.cpp -- a stand-alone program over hostsim.cpp for an ASan + UBSan run of the SSAO and blur kernel bodies under
// the constant sets of the guard sweep (TEST INFRASTRUCTURE; no test runs it, nothing loads it into Python):
//   python tests/ssao_guard_cases.py /tmp/guard_constants.bin
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -mfma -fsanitize=address,undefined,float-cast-overflow \
//       -fno-sanitize-recover=all -I include -I crychic_renderer_amd/csrc -I tests/hostsim tests/hostsim/ssao_guards_san_main.cpp \
//       tests/hostsim/hostsim.cpp -o /tmp/ssao_guards_san && /tmp/ssao_guards_san /tmp/guard_constants.bin
// The file holds a count and that many crychic_ssao_constants (tests/ssao_guard_cases.py dump_constants): NaN, inf, 1e30 and 1e12
// constants reach float-to-int conversions and gather addresses, and an index out of range must show here, not on a device.
// Every plane is a heap block of exactly its size, so a read or a write outside one is reported.  Per constant set and frame size
// (ragged tile grids, one frame of several cells of every coarse map): the SSAO pass over the raw plane, over the pairs plane and
// with tap culling must agree with each other, two row strips with the whole map, and the blur chain over strips with the chain
// over the whole map.  Prints the number of calls; exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ssao_core.hpp"

extern "C" {
void hs_ssao_path(const crychic_ssao_constants* cb, const void* normal, const uint32_t* depth, const uint8_t* randvec, uint16_t* ambient,
                  void* edge_base, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, int use_pairs);
void hs_blur_chain(const crychic_ssao_constants* cb, void* edge_base, uint16_t* plane0, uint16_t* plane1, uint32_t W, uint32_t H, int blurCount,
                   uint32_t row0, uint32_t rows, int use_exit, int onesMargin);
int hs_blur_chain_ssao_plane(int blurCount);
void hs_blur_chain_ssao_rows(int blurCount, uint32_t row0, uint32_t rows, uint32_t h2, uint32_t* r0, uint32_t* rn);
void hs_set_stamp(uint32_t stamp);
void hs_set_prep_margin(int margin);
void hs_ssao_guards(const crychic_ssao_constants* cb, uint32_t W, uint32_t H, uint32_t out[7]);
}

static uint32_t g_seed = 2026u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }

struct Frame {
    uint32_t W, H;
    uint32_t* depth; uint16_t* normal; uint8_t* randvec;
};

// sky on the left, noise near the far plane, a band next to the near plane, spikes, holes and depth 0; normals (x, y, -1) with
// a few texels of arbitrary half-float bits (infinities and NaNs among them)
static Frame make_frame(uint32_t W, uint32_t H)
{
    Frame f{ W, H, static_cast<uint32_t*>(std::malloc((size_t)W * H * 4)), static_cast<uint16_t*>(std::malloc((size_t)W * H * 8)),
             static_cast<uint8_t*>(std::malloc(256 * 256 * 4)) };
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            uint32_t d = 0xFFFFFFu;
            if (x >= W / 3 && x < 2 * W / 3) d = 0xFFF000u + (rnd() & 0xFFFu);
            else if (x >= 2 * W / 3) d = (y & 32u) ? (rnd() & 0x3FFFFFu) : 0xE00000u + (rnd() & 0xFFFFu);
            const uint32_t k = rnd() % 97u;
            if (k == 0) d = 0u; else if (k == 1) d = rnd() & 0xFFFFFFu; else if (k == 2) d = 0xFFFFFFu;
            f.depth[(size_t)y * W + x] = d | (rnd() << 24);
            uint16_t* n = f.normal + ((size_t)y * W + x) * 4;
            n[0] = (uint16_t)(0x3000u | (rnd() & 0x83FFu)); n[1] = (uint16_t)(0x3000u | (rnd() & 0x83FFu)); n[2] = 0xBC00u; n[3] = 0u;
            if (rnd() % 61u == 0) n[rnd() % 3u] = (uint16_t)rnd();
            if (rnd() % 211u == 0) n[rnd() % 3u] = (rnd() & 1u) ? 0x7C00u : 0x7E00u;
        }
    for (size_t i = 0; i < 256 * 256 * 4; ++i) f.randvec[i] = (uint8_t)rnd();
    return f;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s constants.bin (python tests/ssao_guard_cases.py constants.bin)\n", argv[0]); return 2; }
    FILE* fp = std::fopen(argv[1], "rb");
    uint32_t count = 0;
    if (!fp || std::fread(&count, 4, 1, fp) != 1 || count == 0 || count > 4096) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    crychic_ssao_constants* sets = static_cast<crychic_ssao_constants*>(std::malloc(sizeof(crychic_ssao_constants) * count));
    if (std::fread(sets, sizeof(crychic_ssao_constants), count, fp) != count) { std::fprintf(stderr, "%s is short\n", argv[1]); return 2; }
    std::fclose(fp);
    const uint32_t sizes[][2] = { { 130, 34 }, { 322, 190 }, { 516, 132 } };
    long calls = 0;
    uint32_t seen[5][2] = {};
    for (const auto& sz : sizes) {
        const uint32_t W = sz[0], H = sz[1], w2 = W / 2, h2 = H / 2;
        const Frame f = make_frame(W, H);
        const size_t eb = cry::edge_plane_bytes(W, H), ab = (size_t)w2 * h2 * 2;
        for (uint32_t s = 0; s < count; ++s) {
            if (W * H > 50000u && (s % 3u) != (W % 3u)) continue;             // the larger frames: every third set each
            crychic_ssao_constants cb = sets[s];
            cb.InvRenderTargetSize[0] = 1.0f / (float)w2; cb.InvRenderTargetSize[1] = 1.0f / (float)h2;
            uint32_t g[7];
            hs_ssao_guards(&cb, W, H, g);
            const uint32_t which[5] = { g[0], g[1], g[4], g[5], g[6] };
            for (int k = 0; k < 5; ++k) seen[k][which[k] ? 1 : 0]++;
            uint16_t* whole[3];
            for (int mode = 0; mode < 3; ++mode) {                               // raw plane, pairs + culling, pairs alone
                void* edge = std::malloc(eb);
                std::memset(edge, 0xFF, eb);
                whole[mode] = static_cast<uint16_t*>(std::malloc(ab));
                std::memset(whole[mode], 0xA5, ab);
                hs_set_stamp(100u + s); hs_set_prep_margin(-1);
                hs_ssao_path(&cb, f.normal, f.depth, f.randvec, whole[mode], edge, W, H, 0, h2, mode);
                ++calls;
                std::free(edge);
                if (mode && std::memcmp(whole[mode], whole[0], ab) != 0) { std::fprintf(stderr, "set %u at %ux%u: path %d differs from the raw plane's\n", s, W, H, mode); return 1; }
            }
            const uint32_t strips[][2] = { { 0, h2 / 8 + 1 }, { h2 / 3 + 1, h2 / 5 + 1 } };
            // the chain: whole map, then strips on a workspace a previous frame left behind
            const int blurCount = 3;
            void* edge = std::malloc(eb);
            std::memset(edge, 0xFF, eb);
            uint16_t* ref = nullptr;
            for (int part = 0; part < 3; ++part) {
                const uint32_t row0 = part ? strips[part - 1][0] : 0u, rows = part ? strips[part - 1][1] : h2;
                if (part) {
                    uint16_t* a = static_cast<uint16_t*>(std::malloc(ab));
                    std::memset(a, 0xA5, ab);
                    hs_set_stamp(300u + s); hs_set_prep_margin(part == 1 ? 8 : -1);
                    hs_ssao_path(&cb, f.normal, f.depth, f.randvec, a, edge, W, H, row0, rows, 1);
                    ++calls;
                    if (std::memcmp(a + (size_t)row0 * w2, whole[0] + (size_t)row0 * w2, (size_t)rows * w2 * 2) != 0) { std::fprintf(stderr, "set %u at %ux%u: strip %u differs\n", s, W, H, row0); return 1; }
                    std::free(a);
                }
                uint32_t r0, rn;
                hs_blur_chain_ssao_rows(blurCount, row0, rows, h2, &r0, &rn);
                uint16_t* planes[2] = { static_cast<uint16_t*>(std::malloc(ab)), static_cast<uint16_t*>(std::malloc(ab)) };
                std::memset(planes[0], 0xCD, ab); std::memset(planes[1], 0xCD, ab);
                hs_set_stamp(500u + 3u * s + (uint32_t)part); hs_set_prep_margin(-1);
                hs_ssao_path(&cb, f.normal, f.depth, f.randvec, planes[hs_blur_chain_ssao_plane(blurCount)], edge, W, H, r0, rn, 1);
                hs_blur_chain(&cb, edge, planes[0], planes[1], W, H, blurCount, row0, rows, 1, 5 * blurCount);
                calls += 2;
                if (!part) ref = planes[0];
                else {
                    if (std::memcmp(planes[0] + (size_t)row0 * w2, ref + (size_t)row0 * w2, (size_t)rows * w2 * 2) != 0) { std::fprintf(stderr, "set %u at %ux%u: chain strip %u differs\n", s, W, H, row0); return 1; }
                    std::free(planes[0]);
                }
                std::free(planes[1]);
            }
            std::free(ref); std::free(edge);
            for (int mode = 0; mode < 3; ++mode) std::free(whole[mode]);
        }
        std::free(f.depth); std::free(f.normal); std::free(f.randvec);
    }
    std::free(sets);
    for (int k = 0; k < 5; ++k)
        if (!seen[k][0] || !seen[k][1]) { std::fprintf(stderr, "guard %d never took both values\n", k); return 1; }
    std::printf("ssao guards sanitizer run ok: %u constant sets, %ld calls\n", count, calls);
    return 0;
}
