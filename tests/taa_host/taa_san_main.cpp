// taa_san_main.cpp -- a stand-alone program over taa_host.cpp and the checker for an ASan + UBSan run of the kernel body (TEST
// INFRASTRUCTURE):
//   clang -O1 -g -std=c99 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/taa_ref/taa_ref.c -o /tmp/taa_ref.o
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -I crychic_renderer_amd/csrc tests/taa_host/taa_san_main.cpp tests/taa_host/taa_host.cpp /tmp/taa_ref.o -o /tmp/taa_san && /tmp/taa_san
// Every plane is a heap block of exactly its size (the frame planes also 4 bytes and the history planes 8 bytes past the block's
// start), so a read or a write outside one is reported.  The corpus's frame sizes over depth planes of 0, of 0xFFFFFF, of noise and
// with one texel of every 8 x 8 tile different, histories of any uint16, and matrices built here: identical, a sub-pixel and a large
// translation, a shear that varies with depth, a previous w that is negative for part of the depth range, and non-finite products
// (an InvViewProj with a zero w row).  The host body and the checker must agree on both outputs, whole frames and stitched row
// ranges.  Prints the number of calls; exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" uint32_t tah_taa(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, const uint8_t* in,
                            const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                            uint32_t blend, uint32_t flags);
extern "C" void taa_ref(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, const uint8_t* in,
                        const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                        uint32_t blend, uint32_t flags, uint8_t* branch);

static uint32_t g_seed = 2024u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 2 }, { 31, 7 }, { 32, 8 }, { 33, 9 }, { 33, 7 }, { 31, 9 }, { 70, 38 }, { 131, 67 }, { 45, 190 } };
    const uint32_t blends[] = { 26, 1, 256, 128 };
    const uint32_t flagSets[] = { 0, 2, 1, 3 };
    long calls = 0;
    int variant = 0;
    for (const auto& sz : sizes)
        for (int motion = 0; motion < 6; ++motion)
            for (int depthKind = 0; depthKind < 4; ++depthKind) {
                const uint32_t W = sz[0], H = sz[1];
                ++variant;
                const uint32_t blend = blends[variant % 4], flags = flagSets[(variant / 4) % 4];
                const bool reset = (flags & 1u) != 0u;
                float ivp[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                float cur[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                float prev[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                if (motion == 1) { prev[3] = 0.7f / (float)W; prev[7] = -0.3f / (float)H; }            // sub-pixel
                if (motion == 2) { prev[3] = 1.3f; prev[7] = 0.4f; }                                    // most of the frame leaves the history
                if (motion == 3) { prev[2] = 0.11f; prev[6] = -0.07f; cur[2] = 0.01f; }                 // varies with depth
                if (motion == 4) { prev[14] = -2.0f; }                                                  // w = 1 - 2 d: behind for d > 0.5
                if (motion == 5) { ivp[15] = 0.0f; }                                                    // h.w = 0: rw is infinite, P is inf or NaN
                const size_t px = (size_t)W * H;
                uint32_t* depthBlock = static_cast<uint32_t*>(std::malloc(px * 4 + 4));
                uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4));
                uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4));
                uint16_t* hinBlock = static_cast<uint16_t*>(std::malloc(px * 8 + 8));
                uint16_t* houtBlock = static_cast<uint16_t*>(std::malloc(px * 8 + 8));
                uint8_t* refOut = static_cast<uint8_t*>(std::malloc(px * 4));
                uint16_t* refHist = static_cast<uint16_t*>(std::malloc(px * 8));
                const int shift = variant & 1;                             // planes at the block's start, or one texel past it
                uint32_t* depth = depthBlock + shift;
                uint8_t* in = inBlock + 4 * shift;
                uint8_t* out = outBlock + 4 * shift;
                uint16_t* hin = hinBlock + 4 * shift;
                uint16_t* hout = houtBlock + 4 * shift;
                for (uint32_t y = 0; y < H; ++y)
                    for (uint32_t x = 0; x < W; ++x) {
                        const bool odd = (x & 7u) == 3u && (y & 7u) == 5u;
                        depth[(size_t)y * W + x] = depthKind == 0 ? 0u : (depthKind == 1 ? 0xFFFFFFu : (depthKind == 2 ? rnd() : (odd ? 0xFFFFFFu : 0u)));
                    }
                for (size_t i = 0; i < px * 4; ++i) { in[i] = (uint8_t)rnd(); hin[i] = (uint16_t)rnd(); }
                const uint16_t* history = reset && (variant & 2) ? nullptr : hin;
                std::memset(refOut, 0xA5, px * 4);
                std::memset(refHist, 0xA5, px * 8);
                taa_ref(ivp, cur, prev, depth, in, history, refHist, refOut, W, H, 0, H, blend, flags, nullptr);
                std::memset(out, 0xA5, px * 4);
                std::memset(hout, 0xA5, px * 8);
                tah_taa(ivp, cur, prev, depth, in, history, hout, out, W, H, 0, H, blend, flags);
                calls += 2;
                if (std::memcmp(out, refOut, px * 4) != 0 || std::memcmp(hout, refHist, px * 8) != 0) {
                    std::fprintf(stderr, "the host body and the checker differ at %ux%u variant %d\n", W, H, variant);
                    return 1;
                }
                // row ranges, odd starts and single rows included
                const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3 | 1u, H };
                std::memset(out, 0xA5, px * 4);
                std::memset(hout, 0xA5, px * 8);
                for (int c = 0; c + 1 < 6; ++c) {
                    const uint32_t r0 = cuts[c] < H ? cuts[c] : H, r1 = cuts[c + 1] < H ? cuts[c + 1] : H;
                    if (r1 <= r0) continue;
                    tah_taa(ivp, cur, prev, depth, in, history, hout, out, W, H, r0, r1 - r0, blend, flags);
                    ++calls;
                }
                if (std::memcmp(out, refOut, px * 4) != 0 || std::memcmp(hout, refHist, px * 8) != 0) {
                    std::fprintf(stderr, "stitched ranges differ at %ux%u variant %d\n", W, H, variant);
                    return 1;
                }
                std::free(depthBlock); std::free(inBlock); std::free(outBlock); std::free(hinBlock); std::free(houtBlock); std::free(refOut); std::free(refHist);
            }
    std::printf("temporal anti-aliasing sanitizer run ok: %ld calls\n", calls);
    return 0;
}
