// motion_blur_san_main.cpp -- a stand-alone program over motion_blur_host.cpp and the checker for an ASan + UBSan run of the kernel
// bodies (TEST INFRASTRUCTURE; tools/sanitize.sh builds and runs it):
//   clang -O1 -g -std=c99 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/motion_blur_ref/motion_blur_ref.c -o ref.o
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -I crychic_renderer_amd/csrc tests/motion_blur_host/motion_blur_san_main.cpp tests/motion_blur_host/motion_blur_host.cpp ref.o -o san && ./san
// Every plane is a heap block of exactly its size (the frame planes also 4 bytes and the workspace 8 bytes past the block's start), so
// a read or a write outside one is reported.  The corpus's frame sizes and a tall one over depth planes of 0, of 0xFFFFFF, of noise and
// in bands, and matrices built here: identical, a sub-pixel, a several-pixel and a clamped translation, a shear that varies with depth,
// a previous w that is negative for part of the depth range, non-finite products (an InvViewProj with a zero w row) and NaN and
// infinity in the matrices themselves.  The host bodies and the checker must agree on the workspace and the frame, whole frames and
// stitched row ranges.  Prints the number of calls; exits non-zero on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" uint32_t mbh_velocity(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, uint32_t W, uint32_t H,
                                 uint32_t shutter, uint32_t maxRadius, void* workspace);
extern "C" uint32_t mbh_gather(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t samples, const void* workspace);
extern "C" uint64_t mbh_workspace_bytes(uint32_t W, uint32_t H);
extern "C" void motion_blur_ref_velocity(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, uint32_t W,
                                         uint32_t H, uint32_t shutter, uint32_t R, uint32_t* workspace, uint8_t* branch);
extern "C" void motion_blur_ref_gather(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t N,
                                       const uint32_t* workspace, uint8_t* branch);

static uint32_t g_seed = 2025u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 17, 1 }, { 16, 16 }, { 33, 49 }, { 70, 38 }, { 45, 190 } };
    const uint32_t samples[] = { 2, 4, 8, 16, 32 }, radii[] = { 1, 16, 32 }, shutters[] = { 0, 1, 128, 256 };
    long calls = 0;
    int variant = 0;
    for (const auto& sz : sizes)
        for (int motion = 0; motion < 9; ++motion)
            for (int depthKind = 0; depthKind < 4; ++depthKind) {
                const uint32_t W = sz[0], H = sz[1];
                ++variant;
                const uint32_t N = samples[variant % 5], R = radii[variant % 3], shutter = shutters[(variant + variant / 4) % 4];
                float ivp[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                float cur[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                float prev[16] = { 1, 0, 0, 0,  0, 1, 0, 0,  0, 0, 1, 0,  0, 0, 0, 1 };
                if (motion == 1) { prev[3] = 0.7f / (float)W; prev[7] = -0.3f / (float)H; }            // sub-pixel
                if (motion == 2) { prev[3] = 9.0f / (float)W; prev[7] = 5.0f / (float)H; }              // several pixels
                if (motion == 3) { prev[3] = 1.3f; prev[7] = -0.4f; }                                   // clamped at any R
                if (motion == 4) { prev[2] = 0.31f; prev[6] = -0.17f; cur[2] = 0.01f; }                 // varies with depth
                if (motion == 5) { prev[14] = -2.0f; prev[3] = 0.2f; }                                  // w = 1 - 2 d: behind for d > 0.5
                if (motion == 6) { ivp[15] = 0.0f; }                                                    // h.w = 0: rw is infinite, P is inf or NaN
                if (motion == 7) { prev[12] = NAN; cur[5] = INFINITY; }
                if (motion == 8) { cur[0] = 3.0e38f; prev[0] = -3.0e38f; }                              // finite matrices, an infinite difference
                const size_t px = (size_t)W * H, wsBytes = (size_t)mbh_workspace_bytes(W, H);
                uint32_t* depthBlock = static_cast<uint32_t*>(std::malloc(px * 4 + 4));
                uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4));
                uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4));
                uint8_t* wsBlock = static_cast<uint8_t*>(std::malloc(wsBytes + 8));
                uint8_t* refOut = static_cast<uint8_t*>(std::malloc(px * 4));
                uint32_t* refWs = static_cast<uint32_t*>(std::malloc(wsBytes));
                const int shift = variant & 1;                             // planes at the block's start, or one texel past it
                uint32_t* depth = depthBlock + shift;
                uint8_t* in = inBlock + 4 * shift;
                uint8_t* out = outBlock + 4 * shift;
                uint8_t* ws = wsBlock + 8 * shift;
                for (uint32_t y = 0; y < H; ++y)
                    for (uint32_t x = 0; x < W; ++x)
                        depth[(size_t)y * W + x] = depthKind == 0 ? 0u : (depthKind == 1 ? 0xFFFFFFu : (depthKind == 2 ? rnd() : ((x / 5u) & 1u ? 0xFFFFFFu : 0x400000u)));
                for (size_t i = 0; i < px * 4; ++i) in[i] = (uint8_t)rnd();
                std::memset(refOut, 0xA5, px * 4);
                std::memset(refWs, 0xA5, wsBytes);
                motion_blur_ref_velocity(ivp, cur, prev, depth, W, H, shutter, R, refWs, nullptr);
                motion_blur_ref_gather(in, refOut, W, H, 0, H, N, refWs, nullptr);
                std::memset(out, 0xA5, px * 4);
                std::memset(ws, 0xA5, wsBytes);
                mbh_velocity(ivp, cur, prev, depth, W, H, shutter, R, ws);
                mbh_gather(in, out, W, H, 0, H, N, ws);
                calls += 4;
                if (std::memcmp(ws, refWs, wsBytes) != 0 || std::memcmp(out, refOut, px * 4) != 0) {
                    std::fprintf(stderr, "the host bodies and the checker differ at %ux%u variant %d\n", W, H, variant);
                    return 1;
                }
                // row ranges, odd starts, single rows and a cut on a tile's edge included
                const uint32_t cuts[] = { 0, 1, 16, H / 3 + 1, (2 * H) / 3 | 1u, H };
                std::memset(out, 0xA5, px * 4);
                uint32_t last = 0;
                for (int c = 1; c < 6; ++c) {
                    const uint32_t r1 = cuts[c] < H ? cuts[c] : H;
                    if (r1 <= last) continue;
                    mbh_gather(in, out, W, H, last, r1 - last, N, ws);
                    last = r1;
                    ++calls;
                }
                if (std::memcmp(out, refOut, px * 4) != 0) {
                    std::fprintf(stderr, "stitched ranges differ at %ux%u variant %d\n", W, H, variant);
                    return 1;
                }
                std::free(depthBlock); std::free(inBlock); std::free(outBlock); std::free(wsBlock); std::free(refOut); std::free(refWs);
            }
    std::printf("motion blur sanitizer run ok: %ld calls\n", calls);
    return 0;
}
