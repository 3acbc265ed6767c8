// dof_san_main.cpp -- a stand-alone program over dof_host.cpp for an ASan + UBSan run of the kernel body (TEST INFRASTRUCTURE):
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I crychic_renderer_amd/csrc tests/dof_host/dof_san_main.cpp tests/dof_host/dof_host.cpp -o /tmp/dof_san && /tmp/dof_san
// Every plane is a heap block of exactly its size (or 4 bytes more, the plane then 4 bytes past the block's start), so a read or a
// write outside one is reported.  The corpus's frame sizes, every R of 1 .. 8 and four apertures over depth planes of 0, of 0xFFFFFF,
// of noise and of the half-plane step, under two projections and one whose g overflows; whole frames and row ranges must agree, and
// aperture 0 must copy.  Prints the number of calls; exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" uint32_t dfh_dof(const float* proj, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                            uint32_t rows, const uint32_t* params);

static uint32_t g_seed = 2025u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }
static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 5 }, { 63, 4 }, { 64, 4 }, { 65, 7 }, { 130, 9 }, { 322, 190 } };
    const float apertures[] = { 0.0f, 0.5f, 6.0f, 64.0f };
    const float focuses[] = { 2.0f, 15.0f, 90.0f, 3.0e38f };
    const float ab[][2] = { { 1.01010096f, -1.01010096f }, { 1.001001f, -0.5005005f }, { 1.01010096f, -1.0e-3f } };
    long calls = 0;
    int variant = 0;
    for (const auto& sz : sizes)
        for (uint32_t R = 1; R <= 8; ++R)
            for (float aperture : apertures) {
                const uint32_t W = sz[0], H = sz[1];
                ++variant;
                if (W * H > 10000u && (variant % 4) != 0) continue;         // the large frame: every fourth combination
                const int depthKind = variant % 4, cam = (variant / 4) % 3;
                float proj[16] = { 0 };
                proj[10] = ab[cam][0];
                proj[11] = ab[cam][1];
                const uint32_t params[3] = { fbits(focuses[(variant / 3) % 4]), fbits(aperture), R };
                const size_t px = (size_t)W * H;
                const int shift = variant & 1;                             // planes at the block's start, or 4 bytes past it
                uint32_t* depthBlock = static_cast<uint32_t*>(std::malloc(px * 4 + 4 * shift));
                uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4 * shift));
                uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4 * shift));
                uint8_t* ref = static_cast<uint8_t*>(std::malloc(px * 4));
                uint32_t* depth = depthBlock + shift;
                uint8_t* in = inBlock + 4 * shift;
                uint8_t* out = outBlock + 4 * shift;
                for (uint32_t y = 0; y < H; ++y)
                    for (uint32_t x = 0; x < W; ++x)
                        depth[(size_t)y * W + x] = depthKind == 0 ? 0u : (depthKind == 1 ? 0xFFFFFFu : (depthKind == 2 ? rnd() : (x >= W / 2 ? 0xFFFFFFu : 0xE8BA2Eu)));
                for (size_t i = 0; i < px * 4; ++i) in[i] = (uint8_t)rnd();
                std::memset(ref, 0xA5, px * 4);
                dfh_dof(proj, depth, in, ref, W, H, 0, H, params);
                ++calls;
                // row ranges, odd starts and single rows included
                const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3 | 1u, H };
                std::memset(out, 0xA5, px * 4);
                for (int c = 0; c + 1 < 6; ++c) {
                    const uint32_t r0 = cuts[c] < H ? cuts[c] : H, r1 = cuts[c + 1] < H ? cuts[c + 1] : H;
                    if (r1 <= r0) continue;
                    dfh_dof(proj, depth, in, out, W, H, r0, r1 - r0, params);
                    ++calls;
                }
                if (std::memcmp(out, ref, px * 4) != 0) { std::fprintf(stderr, "stitched ranges differ at %ux%u variant %d\n", W, H, variant); return 1; }
                if (aperture == 0.0f && std::memcmp(ref, in, px * 4) != 0) { std::fprintf(stderr, "aperture 0 is not a copy at %ux%u\n", W, H); return 1; }
                std::free(depthBlock); std::free(inBlock); std::free(outBlock); std::free(ref);
            }
    std::printf("dof sanitizer run ok: %ld calls\n", calls);
    return 0;
}
