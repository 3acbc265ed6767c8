// grade_san_main.cpp -- a stand-alone program over grade_host.cpp, the checker and the .cube loader of csrc/host_textures.cpp for an
// ASan + UBSan run (TEST INFRASTRUCTURE; tools/sanitize_grade.sh builds and runs it; CPU only):
//   clang -O1 -g -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/grade_ref/grade_ref.c -o ref.o
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -I include \
//       -I crychic_renderer_amd/csrc tests/grade_host/grade_san_main.cpp tests/grade_host/grade_host.cpp \
//       crychic_renderer_amd/csrc/host_textures.cpp ref.o -o san && ./san <an empty directory>
// The parser runs on hostile files written into the directory -- truncated, a huge N, a line of a megabyte, binary garbage, numbers
// that overflow -- into a heap block of exactly the capacity it is told, and must answer each with an error code.  The kernel's body
// runs on frames and tables that are heap blocks of exactly their size, at every 4-byte misalignment of `in` and `out`, in place and
// in row ranges, and must agree with the checker.  Prints the number of calls; exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "crychic_hip.h"

extern "C" void gh_grade(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint8_t* lut, uint32_t N,
                         uint32_t cus, uint32_t* stats);
extern "C" void gh_build_lut(const float* params, uint32_t N, uint8_t* lut);
extern "C" void grade_ref(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint8_t* lut, uint32_t N);

static uint32_t g_seed = 2031u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }

static std::string g_dir;
static long g_calls = 0;

// The loader's status for a file of `text`, read into a block of exactly `capacity` bytes (0: no block, the size alone).
static int load(const std::string& text, size_t capacity, uint32_t* N)
{
    const std::string path = g_dir + "/hostile.cube";
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
    uint8_t* block = capacity ? static_cast<uint8_t*>(std::malloc(capacity)) : nullptr;
    const int rc = crychic_load_cube_lut(path.c_str(), block, capacity, N);
    std::free(block);
    ++g_calls;
    return rc;
}

static std::string rows(uint32_t n) { std::string s; for (uint32_t i = 0; i < n; ++i) s += "0.25 0.5 0.75\n"; return s; }

static int parser()
{
    uint32_t N = 0;
    int bad = 0;
    // what must load, into exactly 4 N^3 bytes
    bad += load("LUT_3D_SIZE 2\n" + rows(8), 32, &N) != 0 || N != 2u;
    bad += load("# c\r\nTITLE \"t\"\r\nDOMAIN_MIN 0 0 0\r\nDOMAIN_MAX 1 1 1\r\nLUT_3D_SIZE 3\r\n" + rows(27), 108, &N) != 0 || N != 3u;
    bad += load("LUT_3D_SIZE 33\n" + rows(35937), 143748, &N) != 0 || N != 33u;
    bad += load("LUT_3D_SIZE 33\n" + rows(35937), 0, &N) != 0 || N != 33u;
    if (bad) { std::fprintf(stderr, "a good file was refused\n"); return 1; }
    // what must be refused
    const std::string hostile[] = {
        "", "LUT_3D_SIZE", "LUT_3D_SIZE 2", "LUT_3D_SIZE 2\n" + rows(7), "LUT_3D_SIZE 2\n" + rows(7) + "0.25 0.5", "LUT_3D_SIZE 2\n" + rows(9),
        "LUT_3D_SIZE 4000000000\n" + rows(8), "LUT_3D_SIZE 1e30\n" + rows(8), "LUT_3D_SIZE -5\n" + rows(8), "LUT_3D_SIZE 34\n" + rows(8),
        "LUT_3D_SIZE 99999999999999999999999999999999999999999999\n", "LUT_1D_SIZE 2\n" + rows(2), "DOMAIN_MAX 1 1\nLUT_3D_SIZE 2\n" + rows(8),
        "LUT_3D_SIZE 2\n" + std::string(1u << 20, '7') + "\n" + rows(8), "LUT_3D_SIZE 2\n#" + std::string(1u << 20, ' '),
        "LUT_3D_SIZE 2\n" + rows(7) + "1e999 0 0\n", "LUT_3D_SIZE 2\n" + rows(7) + "0 0 0x1p+\n", "LUT_3D_SIZE 2\n" + rows(7) + "- + .\n",
        std::string("LUT_3D_SIZE 2\n0 0 \0 0\n", 21) + rows(7), "LUT_3D_SIZE 2\n" + rows(3) + "LUT_3D_SIZE 3\n" + rows(5),
    };
    for (const std::string& text : hostile) {
        if (load(text, 32, &N) >= 0) { std::fprintf(stderr, "a hostile file was accepted: %.40s\n", text.c_str()); return 1; }
        if (load(text, 0, &N) >= 0) { std::fprintf(stderr, "a hostile file was accepted without a table: %.40s\n", text.c_str()); return 1; }
    }
    if (load("LUT_3D_SIZE 2\n" + rows(8), 31, &N) >= 0) { std::fprintf(stderr, "a capacity of 31 bytes was accepted\n"); return 1; }
    if (load("LUT_3D_SIZE 33\n" + rows(35937), 143747, &N) >= 0) { std::fprintf(stderr, "a capacity one byte short was accepted\n"); return 1; }
    // binary garbage of several lengths, with and without newlines
    for (int k = 0; k < 64; ++k) {
        std::string g(1u + rnd() % 5000u, '\0');
        for (char& c : g) c = (char)(k & 1 ? rnd() : (rnd() % 3u ? rnd() : '\n'));
        if (load(g, 32, &N) >= 0) { std::fprintf(stderr, "binary garbage was accepted\n"); return 1; }
    }
    if (crychic_load_cube_lut(nullptr, nullptr, 0, &N) >= 0 || crychic_load_cube_lut((g_dir + "/none.cube").c_str(), nullptr, 0, &N) >= 0) return 1;
    std::remove((g_dir + "/hostile.cube").c_str());
    return 0;
}

static int body()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 1 }, { 5, 3 }, { 67, 5 }, { 128, 96 }, { 4100, 3 } };
    const uint32_t Ns[] = { 2, 3, 16, 17, 32, 33 };
    int variant = 0;
    for (const auto& sz : sizes)
        for (const uint32_t N : Ns) {
            const uint32_t W = sz[0], H = sz[1];
            const size_t bytes = (size_t)W * H * 4, lutBytes = (size_t)4 * N * N * N;
            uint8_t* lut = static_cast<uint8_t*>(std::malloc(lutBytes));
            if (variant % 3 == 0) {
                const float p[10] = { 1.2f, 1.0f, 0.8f, 0.03f, 0.0f, -0.02f, 0.9f, 1.0f, 1.2f, 1.3f };
                gh_build_lut(p, N, lut);
            } else {
                for (size_t i = 0; i < lutBytes; ++i) lut[i] = (uint8_t)rnd();
            }
            uint8_t* ref = static_cast<uint8_t*>(std::malloc(bytes));
            for (uint32_t inShift = 0; inShift < 16; inShift += 4)
                for (uint32_t outShift = 0; outShift < 16; outShift += 4) {
                    ++variant;
                    if (W * H > 10000u && inShift != outShift && (variant % 3) != 0) continue;
                    // malloc returns 16-byte aligned blocks: the planes end exactly at their block's end
                    uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(bytes + inShift));
                    uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(bytes + outShift));
                    uint8_t* in = inBlock + inShift;
                    uint8_t* out = outBlock + outShift;
                    for (size_t i = 0; i < bytes; ++i) in[i] = (i % 23u) == 0u ? 255u : (uint8_t)rnd();
                    std::memset(ref, 0xA5, bytes);
                    grade_ref(in, ref, W, H, 0, H, lut, N);
                    std::memset(out, 0xA5, bytes);
                    gh_grade(in, out, W, H, 0, H, lut, N, 2u, nullptr);
                    ++g_calls;
                    if (std::memcmp(out, ref, bytes) != 0) { std::fprintf(stderr, "the host body and the checker differ at %ux%u N %u shifts %u %u\n", W, H, N, inShift, outShift); return 1; }
                    // row ranges, single rows included, stitched
                    std::memset(out, 0xA5, bytes);
                    const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3, H };
                    for (int c = 0; c + 1 < 6; ++c) {
                        const uint32_t r0 = cuts[c] < H ? cuts[c] : H, r1 = cuts[c + 1] < H ? cuts[c + 1] : H;
                        if (r1 <= r0) continue;
                        gh_grade(in, out, W, H, r0, r1 - r0, lut, N, 1u, nullptr);
                        ++g_calls;
                    }
                    if (std::memcmp(out, ref, bytes) != 0) { std::fprintf(stderr, "stitched ranges differ at %ux%u N %u\n", W, H, N); return 1; }
                    if (inShift == outShift) {      // in place
                        gh_grade(in, in, W, H, 0, H, lut, N, 3u, nullptr);
                        ++g_calls;
                        if (std::memcmp(in, ref, bytes) != 0) { std::fprintf(stderr, "in place differs at %ux%u N %u\n", W, H, N); return 1; }
                    }
                    std::free(inBlock); std::free(outBlock);
                }
            std::free(ref); std::free(lut);
        }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: grade_san <an empty directory>\n"); return 2; }
    g_dir = argv[1];
    if (int rc = parser()) return rc;
    if (int rc = body()) return rc;
    std::printf("grade sanitizer run ok: %ld calls\n", g_calls);
    return 0;
}
