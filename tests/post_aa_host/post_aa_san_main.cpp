// post_aa_san_main.cpp -- a stand-alone program over post_aa_host.cpp for an ASan + UBSan run of the kernel body (TEST INFRASTRUCTURE):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I crychic_renderer_amd/csrc \
//       tests/post_aa_host/post_aa_san_main.cpp tests/post_aa_host/post_aa_host.cpp -o /tmp/post_aa_san && /tmp/post_aa_san
// Every plane is a heap block of exactly W * H * 4 bytes (the dword path also on blocks 4 bytes past a 16-byte boundary), and the
// emulated LDS is a heap block of the kernel's size, so a read or write outside a plane or the tile is reported.  Noise, slanted
// two-colour edges and uniform frames at the tile-edge sizes, every parameter set of the tests, whole frames and row ranges; the
// 16-byte and the dword path must agree.  Prints the number of runs; exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int pah_antialias(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint32_t* params,
                             int path);

static uint32_t g_seed = 12345u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static void fill(uint8_t* p, uint32_t W, uint32_t H, int kind)
{
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            uint8_t* t = p + 4 * ((size_t)y * W + x);
            if (kind == 0) for (int c = 0; c < 4; ++c) t[c] = (uint8_t)rnd();
            else if (kind == 1) { const bool s = 5 * y > x + H; t[0] = s ? 230 : 20; t[1] = s ? 220 : 30; t[2] = s ? 40 : 160; t[3] = s ? 255 : 128; }
            else if (kind == 2) { const bool s = 20 * x > y + W; t[0] = t[1] = t[2] = s ? 255 : 0; t[3] = (uint8_t)(x * 7 + y * 13); }
            else t[0] = t[1] = t[2] = t[3] = 93;
        }
}

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 1, 7 }, { 7, 1 }, { 2, 2 }, { 4, 4 }, { 63, 31 }, { 64, 32 }, { 65, 33 }, { 68, 33 }, { 130, 70 }, { 132, 70 }, { 322, 190 }, { 324, 97 } };
    const uint32_t params[][4] = { { 2048, 3, 12, 192 }, { 2048, 3, 1, 192 }, { 2048, 3, 16, 192 }, { 0, 31, 12, 192 }, { 2048, 3, 12, 0 }, { 0, 0, 16, 256 } };
    long runs = 0;
    for (const auto& sz : sizes)
        for (int kind = 0; kind < 4; ++kind)
            for (const auto& pr : params) {
                const uint32_t W = sz[0], H = sz[1];
                const size_t n = (size_t)W * H * 4;
                // malloc's blocks are 16-byte aligned: a width that is a multiple of 4 takes the 16-byte path under the launcher's choice
                uint8_t* in = static_cast<uint8_t*>(std::malloc(n));
                uint8_t* ref = static_cast<uint8_t*>(std::malloc(n));
                uint8_t* out = static_cast<uint8_t*>(std::malloc(n));
                fill(in, W, H, kind);
                std::memset(ref, 0xA5, n);
                if (pah_antialias(in, ref, W, H, 0, H, pr, 2) != 2) return 2;              // the dword path, whole frame
                ++runs;
                std::memset(out, 0xA5, n);
                const int taken = pah_antialias(in, out, W, H, 0, H, pr, 0);                // the launcher's choice
                ++runs;
                if (std::memcmp(out, ref, n) != 0) { std::fprintf(stderr, "path %d differs from the dword path at %ux%u kind %d\n", taken, W, H, kind); return 1; }
                // a block 4 bytes past the allocation's start: never the 16-byte path
                uint8_t* in4 = static_cast<uint8_t*>(std::malloc(n + 4));
                uint8_t* out4 = static_cast<uint8_t*>(std::malloc(n + 4));
                std::memcpy(in4 + 4, in, n);
                if (pah_antialias(in4 + 4, out4 + 4, W, H, 0, H, pr, 0) != 2) return 2;
                ++runs;
                if (std::memcmp(out4 + 4, ref, n) != 0) { std::fprintf(stderr, "misaligned plane differs at %ux%u kind %d\n", W, H, kind); return 1; }
                // row ranges, odd starts and single rows included
                const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3 | 1u, H };
                std::memset(out, 0xA5, n);
                for (int c = 0; c + 1 < 6; ++c) {
                    const uint32_t r0 = cuts[c] < H ? cuts[c] : H, r1 = cuts[c + 1] < H ? cuts[c + 1] : H;
                    if (r1 <= r0) continue;
                    pah_antialias(in, out, W, H, r0, r1 - r0, pr, 0);
                    ++runs;
                }
                if (std::memcmp(out, ref, n) != 0) { std::fprintf(stderr, "stitched ranges differ at %ux%u kind %d\n", W, H, kind); return 1; }
                std::free(in); std::free(ref); std::free(out); std::free(in4); std::free(out4);
            }
    std::printf("post_aa sanitizer run ok: %ld runs\n", runs);
    return 0;
}
