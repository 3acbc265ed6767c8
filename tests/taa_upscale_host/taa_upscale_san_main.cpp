// taa_upscale_san_main.cpp -- a stand-alone program over taa_upscale_host.cpp and the checker for an ASan + UBSan run of the kernel
// body (TEST INFRASTRUCTURE; tools/sanitize_taa_upscale.sh builds and runs it).  Every plane is a heap block of exactly its size (the
// frame planes also 4 bytes and the history planes 8 bytes past the block's start), so a read or a write outside one is reported.  The
// corpus's shapes and a tall one, under jitters at zero, at both ends and in between, over depth planes of 0, of 0xFFFFFF, of noise
// and with one texel of every 8 x 8 tile different, histories of any uint16, and matrices built here: identical, a sub-pixel and a
// large translation, a shear that varies with depth, a previous w that is negative for part of the depth range, and non-finite
// products (an InvViewProj with a zero w row).  The host body and the checker must agree on both outputs, whole frames and stitched
// row ranges.  Prints the number of calls; exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" uint32_t tuh_taa_upscale(const float* invViewProj, const float* curViewProj, const float* prevViewProj, float jx, float jy, const uint32_t* depth,
                                    const uint8_t* in, uint32_t Wi, uint32_t Hi, const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out,
                                    uint32_t Wo, uint32_t Ho, uint32_t row0, uint32_t rows, uint32_t blend, uint32_t flags);
extern "C" void taa_upscale_ref(const float* invViewProj, const float* curViewProj, const float* prevViewProj, float jx, float jy, const uint32_t* depth,
                                const uint8_t* in, uint32_t Wi, uint32_t Hi, const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t Wo,
                                uint32_t Ho, uint32_t row0, uint32_t rows, uint32_t blend, uint32_t flags, uint8_t* branch, uint16_t* weight);

static uint32_t g_seed = 2028u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }

int main()
{
    const uint32_t shapes[][4] = { { 7, 5, 7, 5 }, { 6, 4, 9, 6 }, { 7, 5, 11, 9 }, { 8, 8, 16, 16 }, { 3, 2, 12, 8 }, { 1, 1, 3, 3 }, { 1, 1, 4, 4 },
                                   { 47, 26, 70, 38 }, { 33, 9, 130, 9 }, { 30, 100, 45, 190 } };
    const float jitters[][2] = { { 0.0f, 0.0f }, { 0.5f, -0.5f }, { -0.5f, 0.5f }, { 0.0f, -1.0f / 6.0f }, { -0.25f, 1.0f / 6.0f }, { 0.4999f, -0.4999f } };
    const uint32_t blends[] = { 102, 1, 256, 128 };
    const uint32_t flagSets[] = { 0, 2, 1, 3 };
    long calls = 0;
    int variant = 0;
    for (const auto& sh : shapes)
        for (int motion = 0; motion < 6; ++motion)
            for (int depthKind = 0; depthKind < 4; ++depthKind) {
                const uint32_t Wi = sh[0], Hi = sh[1], Wo = sh[2], Ho = sh[3];
                ++variant;
                const uint32_t blend = blends[variant % 4], flags = flagSets[(variant / 4) % 4];
                const float jx = jitters[variant % 6][0], jy = jitters[variant % 6][1];
                const bool reset = (flags & 1u) != 0u;
                float ivp[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                float cur[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                float prev[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                if (motion == 1) { prev[3] = 0.7f / (float)Wi; prev[7] = -0.3f / (float)Hi; }          // sub-pixel
                if (motion == 2) { prev[3] = 1.3f; prev[7] = 0.4f; }                                    // most of the frame leaves the history
                if (motion == 3) { prev[2] = 0.11f; prev[6] = -0.07f; cur[2] = 0.01f; }                 // varies with depth
                if (motion == 4) { prev[14] = -2.0f; }                                                  // w = 1 - 2 d: behind for d > 0.5
                if (motion == 5) { ivp[15] = 0.0f; }                                                    // h.w = 0: rw is infinite, P is inf or NaN
                const size_t pi = (size_t)Wi * Hi, po = (size_t)Wo * Ho;
                uint32_t* depthBlock = static_cast<uint32_t*>(std::malloc(pi * 4 + 4));
                uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(pi * 4 + 4));
                uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(po * 4 + 4));
                uint16_t* hinBlock = static_cast<uint16_t*>(std::malloc(po * 8 + 8));
                uint16_t* houtBlock = static_cast<uint16_t*>(std::malloc(po * 8 + 8));
                uint8_t* refOut = static_cast<uint8_t*>(std::malloc(po * 4));
                uint16_t* refHist = static_cast<uint16_t*>(std::malloc(po * 8));
                const int shift = variant & 1;                             // planes at the block's start, or one texel past it
                uint32_t* depth = depthBlock + shift;
                uint8_t* in = inBlock + 4 * shift;
                uint8_t* out = outBlock + 4 * shift;
                uint16_t* hin = hinBlock + 4 * shift;
                uint16_t* hout = houtBlock + 4 * shift;
                for (uint32_t y = 0; y < Hi; ++y)
                    for (uint32_t x = 0; x < Wi; ++x) {
                        const bool odd = (x & 7u) == 3u && (y & 7u) == 5u;
                        depth[(size_t)y * Wi + x] = depthKind == 0 ? 0u : (depthKind == 1 ? 0xFFFFFFu : (depthKind == 2 ? rnd() : (odd ? 0xFFFFFFu : 0u)));
                    }
                for (size_t i = 0; i < pi * 4; ++i) in[i] = (uint8_t)rnd();
                for (size_t i = 0; i < po * 4; ++i) hin[i] = (uint16_t)rnd();
                const uint16_t* history = reset && (variant & 2) ? nullptr : hin;
                std::memset(refOut, 0xA5, po * 4);
                std::memset(refHist, 0xA5, po * 8);
                taa_upscale_ref(ivp, cur, prev, jx, jy, depth, in, Wi, Hi, history, refHist, refOut, Wo, Ho, 0, Ho, blend, flags, nullptr, nullptr);
                std::memset(out, 0xA5, po * 4);
                std::memset(hout, 0xA5, po * 8);
                tuh_taa_upscale(ivp, cur, prev, jx, jy, depth, in, Wi, Hi, history, hout, out, Wo, Ho, 0, Ho, blend, flags);
                calls += 2;
                if (std::memcmp(out, refOut, po * 4) != 0 || std::memcmp(hout, refHist, po * 8) != 0) {
                    std::fprintf(stderr, "the host body and the checker differ at %ux%u -> %ux%u variant %d\n", Wi, Hi, Wo, Ho, variant);
                    return 1;
                }
                // row ranges of the output, odd starts and single rows included
                const uint32_t cuts[] = { 0, 1, Ho / 3, Ho / 3 + 1, (2 * Ho) / 3 | 1u, Ho };
                std::memset(out, 0xA5, po * 4);
                std::memset(hout, 0xA5, po * 8);
                for (int c = 0; c + 1 < 6; ++c) {
                    const uint32_t r0 = cuts[c] < Ho ? cuts[c] : Ho, r1 = cuts[c + 1] < Ho ? cuts[c + 1] : Ho;
                    if (r1 <= r0) continue;
                    tuh_taa_upscale(ivp, cur, prev, jx, jy, depth, in, Wi, Hi, history, hout, out, Wo, Ho, r0, r1 - r0, blend, flags);
                    ++calls;
                }
                if (std::memcmp(out, refOut, po * 4) != 0 || std::memcmp(hout, refHist, po * 8) != 0) {
                    std::fprintf(stderr, "stitched ranges differ at %ux%u -> %ux%u variant %d\n", Wi, Hi, Wo, Ho, variant);
                    return 1;
                }
                std::free(depthBlock); std::free(inBlock); std::free(outBlock); std::free(hinBlock); std::free(houtBlock); std::free(refOut); std::free(refHist);
            }
    std::printf("temporal upsampling sanitizer run ok: %ld calls\n", calls);
    return 0;
}
