// bloom_san_main.cpp -- a stand-alone program over bloom_host.cpp for an ASan + UBSan run of the kernel bodies (TEST INFRASTRUCTURE):
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I crychic_renderer_amd/csrc tests/bloom_host/bloom_san_main.cpp tests/bloom_host/bloom_host.cpp -o /tmp/bloom_san && /tmp/bloom_san
// Every plane and the workspace are heap blocks of exactly their size (or the plane 4 bytes past the start of a block 4 bytes larger),
// so a read or a write outside one is reported.  The corpus's frame sizes under every level count of 1 .. 8, four thresholds and the
// ends of scatter, knee and intensity, over noise and over a dim frame with a bright corner; out of place and in place; whole frames
// and row ranges must agree, intensity 0 must copy and nothing may come out darker.  Prints the number of calls; exits non-zero on a
// mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" void bh_bloom(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint32_t* params, uint8_t* workspace,
                         uint32_t what, uint32_t* stats);
extern "C" size_t bh_workspace_bytes(uint32_t W, uint32_t H, uint32_t levels);

static uint32_t g_seed = 2026u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 2, 3 }, { 7, 5 }, { 33, 17 }, { 64, 64 }, { 65, 63 }, { 129, 97 }, { 64, 32 }, { 66, 34 }, { 322, 190 } };
    const uint32_t thresholds[] = { 0, 100, 192, 255 };
    const uint32_t scatters[] = { 0, 179, 256 }, knees[] = { 1, 32, 255 }, intensities[] = { 0, 128, 1024 };
    long calls = 0;
    int variant = 0;
    uint32_t stats[4] = { 0, 0, 0, 0 };
    for (const auto& sz : sizes)
        for (uint32_t levels = 1; levels <= 8; ++levels)
            for (uint32_t T : thresholds) {
                const uint32_t W = sz[0], H = sz[1];
                ++variant;
                if (W * H > 10000u && (variant % 4) != 0) continue;         // the large frame: every fourth combination
                const uint32_t params[5] = { T, knees[variant % 3], scatters[(variant / 3) % 3], intensities[(variant / 2) % 3], levels };
                const size_t px = (size_t)W * H, wsBytes = bh_workspace_bytes(W, H, levels);
                const int shift = variant & 1;                             // planes at the block's start, or 4 bytes past it
                uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4 * shift));
                uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4 * shift));
                uint8_t* ref = static_cast<uint8_t*>(std::malloc(px * 4));
                uint8_t* ws = static_cast<uint8_t*>(std::aligned_alloc(16, (wsBytes + 15) & ~(size_t)15));
                uint8_t* ws2 = static_cast<uint8_t*>(std::malloc(wsBytes));
                uint8_t* in = inBlock + 4 * shift;
                uint8_t* out = outBlock + 4 * shift;
                const bool blob = (variant % 5) == 0;
                for (uint32_t y = 0; y < H; ++y)
                    for (uint32_t x = 0; x < W; ++x)
                        for (int c = 0; c < 4; ++c)
                            in[((size_t)y * W + x) * 4 + c] = (uint8_t)(blob ? (x < W / 3 + 1 && y < H / 3 + 1 ? 230 + rnd() % 26 : rnd() % 120) : rnd());
                std::memset(ref, 0xA5, px * 4);
                std::memset(ws, 0xA5, wsBytes);
                bh_bloom(in, ref, W, H, 0, H, params, ws, 3, stats);
                ++calls;
                std::memcpy(ws2, ws, wsBytes);
                // row ranges behind one pyramid, odd starts and single rows included; the composite must leave the workspace alone
                const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3 | 1u, H };
                std::memset(out, 0xA5, px * 4);
                for (int c = 0; c + 1 < 6; ++c) {
                    const uint32_t r0 = cuts[c] < H ? cuts[c] : H, r1 = cuts[c + 1] < H ? cuts[c + 1] : H;
                    if (r1 <= r0) continue;
                    bh_bloom(in, out, W, H, r0, r1 - r0, params, ws, 2, stats);
                    ++calls;
                }
                if (std::memcmp(out, ref, px * 4) != 0) { std::fprintf(stderr, "stitched ranges differ at %ux%u variant %d\n", W, H, variant); return 1; }
                if (std::memcmp(ws, ws2, wsBytes) != 0) { std::fprintf(stderr, "the composite wrote the workspace at %ux%u variant %d\n", W, H, variant); return 1; }
                if (params[3] == 0u && std::memcmp(ref, in, px * 4) != 0) { std::fprintf(stderr, "intensity 0 is not a copy at %ux%u\n", W, H); return 1; }
                for (size_t i = 0; i < px * 4; ++i)
                    if (ref[i] < in[i]) { std::fprintf(stderr, "a channel came out darker at %ux%u variant %d\n", W, H, variant); return 1; }
                // in place: the pyramid again over a poisoned workspace, then the composite over the input itself
                std::memcpy(out, in, px * 4);
                std::memset(ws, 0x5A, wsBytes);
                bh_bloom(out, out, W, H, 0, H, params, ws, 3, stats);
                ++calls;
                if (std::memcmp(out, ref, px * 4) != 0) { std::fprintf(stderr, "in place differs at %ux%u variant %d\n", W, H, variant); return 1; }
                std::free(inBlock); std::free(outBlock); std::free(ref); std::free(ws); std::free(ws2);
            }
    std::printf("bloom sanitizer run ok: %ld calls (%u workgroups, %u zero tiles, %u silent wavefronts, %u 16-byte composites)\n", calls, stats[0], stats[1],
                stats[2], stats[3]);
    return 0;
}
