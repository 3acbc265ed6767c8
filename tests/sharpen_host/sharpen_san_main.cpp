// sharpen_san_main.cpp -- a stand-alone program over sharpen_host.cpp and the checker for an ASan + UBSan run (TEST INFRASTRUCTURE;
// tools/sanitize_sharpen.sh builds and runs it; CPU only):
//   clang -O1 -g -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/sharpen_ref/sharpen_ref.c -o ref.o
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -I crychic_renderer_amd/csrc tests/sharpen_host/sharpen_san_main.cpp tests/sharpen_host/sharpen_host.cpp ref.o -o san && ./san
// The kernels' bodies run on frames that are heap blocks of exactly their size -- random, extreme-valued, near-flat and flat --, at
// every 4-byte misalignment of `in` and `out`, whole and in row ranges that stitch, and must agree with the checker; a read or a
// write one pixel past a plane, a signed overflow or a float out of an integer's range ends the run.  Prints the number of calls;
// exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" void sh_sharpen(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t strength, uint32_t limit,
                           uint32_t* stats);
extern "C" uint32_t sh_q12_mismatches(int ulps);
extern "C" uint64_t sh_div_mismatches(uint32_t t0, uint32_t t1, int ulps);
extern "C" void sharpen_ref(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t strength, uint32_t limit);

static uint32_t g_seed = 2032u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }
static long g_calls = 0;

static void fill(uint8_t* p, size_t bytes, int kind)
{
    static const uint8_t extreme[8] = { 0, 1, 2, 127, 128, 253, 254, 255 };
    const uint8_t level = (uint8_t)(rnd() % 253u);
    for (size_t i = 0; i < bytes; ++i)
        p[i] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? extreme[rnd() & 7u] : kind == 2 ? (uint8_t)(level + (rnd() & 3u)) : level;
}

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 1, 5 }, { 5, 1 }, { 2, 2 }, { 3, 3 }, { 7, 3 }, { 8, 3 }, { 9, 3 }, { 255, 3 }, { 256, 3 }, { 257, 3 }, { 260, 9 },
                                  { 1023, 2 }, { 1024, 2 }, { 1028, 3 }, { 12, 7 }, { 12, 8 }, { 12, 9 }, { 12, 17 }, { 13, 17 } };
    const uint32_t params[][2] = { { 256, 3072 }, { 128, 3072 }, { 1, 3584 }, { 256, 3584 }, { 0, 3072 }, { 256, 0 } };
    int variant = 0;
    for (const auto& sz : sizes)
        for (int kind = 0; kind < 4; ++kind) {
            const uint32_t W = sz[0], H = sz[1];
            const size_t bytes = (size_t)W * H * 4;
            uint8_t* ref = static_cast<uint8_t*>(std::malloc(bytes));
            for (uint32_t inShift = 0; inShift < 16; inShift += 4)
                for (uint32_t outShift = 0; outShift < 16; outShift += 4) {
                    const uint32_t* p = params[variant++ % 6];
                    if (W * H > 2000u && inShift != outShift) continue;
                    // malloc returns 16-byte aligned blocks: the planes end exactly at their block's end
                    uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(bytes + inShift));
                    uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(bytes + outShift));
                    uint8_t* in = inBlock + inShift;
                    uint8_t* out = outBlock + outShift;
                    fill(in, bytes, kind);
                    std::memset(ref, 0xA5, bytes);
                    sharpen_ref(in, ref, W, H, 0, H, p[0], p[1]);
                    std::memset(out, 0xA5, bytes);
                    sh_sharpen(in, out, W, H, 0, H, p[0], p[1], nullptr);
                    ++g_calls;
                    if (std::memcmp(out, ref, bytes) != 0) { std::fprintf(stderr, "the host body and the checker differ at %ux%u kind %d shifts %u %u\n", W, H, kind, inShift, outShift); return 1; }
                    // row ranges, single rows included, stitched
                    std::memset(out, 0xA5, bytes);
                    const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3, H };
                    for (int c = 0; c + 1 < 6; ++c) {
                        const uint32_t r0 = cuts[c] < H ? cuts[c] : H, r1 = cuts[c + 1] < H ? cuts[c + 1] : H;
                        if (r1 <= r0) continue;
                        sh_sharpen(in, out, W, H, r0, r1 - r0, p[0], p[1], nullptr);
                        ++g_calls;
                    }
                    if (std::memcmp(out, ref, bytes) != 0) { std::fprintf(stderr, "stitched ranges differ at %ux%u kind %d\n", W, H, kind); return 1; }
                    std::free(inBlock); std::free(outBlock);
                }
            std::free(ref);
        }
    // the division routines under float-cast-overflow: the quotients over all pairs, the rounded division over both ends of t
    for (int ulps = -1; ulps <= 1; ++ulps)
        if (sh_q12_mismatches(ulps) || sh_div_mismatches(0, 2, ulps) || sh_div_mismatches(3583, 3585, ulps)) { std::fprintf(stderr, "a division routine is not the floor\n"); return 1; }
    std::printf("sharpen sanitizer run ok: %ld calls\n", g_calls);
    return 0;
}
