// ssr_gloss_san_main.cpp -- a stand-alone program over ssr_gloss_host.cpp and the checker for an ASan + UBSan run of the kernel
// bodies of crychic_ssr_pyramid and crychic_ssr_glossy (TEST INFRASTRUCTURE; tools/sanitize_ssr_gloss.sh builds and runs it):
//   clang -O1 -g -std=c99 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/ssr_gloss_ref/ssr_gloss_ref.c -o ref.o
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -I include -I crychic_renderer_amd/csrc tests/ssr_gloss_host/ssr_gloss_san_main.cpp tests/ssr_gloss_host/ssr_gloss_host.cpp ref.o -o san && ./san
// Every plane is a heap block of exactly its size (the frame and depth planes also 4 bytes past the block's start), the pyramid a
// 16-byte aligned block of exactly crychic_ssr_pyramid_bytes as the checker's plan gives them (one byte where that is 0), so a read or
// a write outside one is reported, and a float that does not fit its integer is reported where it is converted.  The three gloss
// settings of the corpus in turn; the host pyramid must equal the checker's on every byte of every level.  The corpus's frame
// sizes, a wide and a tall one, step counts and parameter sets over depth planes of 0, of 0xFFFFFF, of noise and a floor's ramp, under
// a camera built here (an eye at (0, 2, -15) looking along +z), with G-buffers of noise, of a floor, with normals of zero length and
// with NaN and infinities, and with non-finite entries in ViewProj.  The host body and the checker must agree on whole frames and on
// stitched row ranges.  Prints the number of calls; exits non-zero on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" uint32_t ssgh_pyramid(const uint8_t* in, uint32_t W, uint32_t H, uint32_t levels, uint8_t* workspace);
extern "C" uint32_t ssgh_glossy(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, const float* nearZ,
                                const void* g0, const void* g1, const void* g2, const uint32_t* depth, const uint8_t* in, const void* pyramid,
                                uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t formatFlags, const uint32_t* params,
                                const uint32_t* gloss);
extern "C" uint32_t ssr_gloss_plan_ref(uint32_t W, uint32_t H, uint32_t levels, uint64_t* sizes);
extern "C" void ssr_gloss_pyramid_ref(const uint8_t* in, uint32_t W, uint32_t H, uint32_t levels, uint8_t* workspace);
extern "C" void ssr_gloss_ref(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, const float* nearZ, const float* g0,
                              const float* g1, const float* g2, const uint32_t* depth, const uint8_t* in, const uint8_t* pyramid, uint8_t* out,
                              uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint32_t* params, const uint32_t* gloss, uint64_t* counters,
                              int32_t* debug);

static uint8_t* block16(size_t n)
{
    void* p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1)) std::abort();
    return static_cast<uint8_t*>(p);
}

static uint32_t g_seed = 2027u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }
static float unit() { return (float)(rnd() >> 8) / 16777216.0f; }
static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 5 }, { 63, 4 }, { 64, 4 }, { 65, 7 }, { 130, 9 }, { 322, 190 }, { 4100, 3 }, { 3, 4100 } };
    // maxDistance, thickness, bias, maxRoughness, steps, edgeFade, intensity, reserved
    const uint32_t params[][8] = { { fbits(20.0f), fbits(0.5f), fbits(0.02f), fbits(0.75f), 32, 32, 256, 0 }, { fbits(5.0f), fbits(0.5f), fbits(0.02f), fbits(0.75f), 1, 32, 256, 0 },
                                   { fbits(20.0f), fbits(8.0f), fbits(0.02f), fbits(0.75f), 2, 4, 256, 0 }, { fbits(120.0f), fbits(0.5f), fbits(0.0f), fbits(0.75f), 63, 1024, 128, 0 },
                                   { fbits(30.0f), fbits(50.0f), fbits(0.001f), fbits(1.0f), 64, 4, 256, 0 } };
    // coneScale, levels, reserved
    const uint32_t gloss[][4] = { { fbits(0.0f), 6, 0, 0 }, { fbits(0.5f), 3, 0, 0 }, { fbits(16.0f), 8, 0, 0 } };
    long calls = 0;
    int variant = 0;
    for (const auto& sz : sizes)
        for (const auto& pr : params)
            for (int gKind = 0; gKind < 4; ++gKind) {
                const uint32_t W = sz[0], H = sz[1];
                ++variant;
                if (W * H > 10000u && (variant % 4) != 0) continue;         // the large frames: every fourth combination
                const int depthKind = variant % 4, camKind = (variant / 4) % 5;
                // the camera, matrices stored transposed (column c of the row-vector matrix at floats 4c ..)
                const float n = 1.0f, f = 100.0f, tanv = 0.41421356f, aspect = (float)W / (float)H;
                const float eye[3] = { 0.0f, 2.0f, -15.0f };
                const float A = f / (f - n), B = -n * f / (f - n), sx = 1.0f / (aspect * tanv), sy = 1.0f / tanv;
                float proj[16] = { sx, 0, 0, 0,  0, sy, 0, 0,  0, 0, A, B,  0, 0, 1, 0 };
                float vp[16] = { sx, 0, 0, -eye[0] * sx,  0, sy, 0, -eye[1] * sy,  0, 0, A, B - eye[2] * A,  0, 0, 1, -eye[2] };
                const float wz = -(f - n) / (n * f), ww = 1.0f / n;
                float ivp[16] = { aspect * tanv, 0, eye[0] * wz, eye[0] * ww,  0, tanv, eye[1] * wz, eye[1] * ww,  0, 0, eye[2] * wz, 1.0f + eye[2] * ww,  0, 0, wz, ww };
                float nearZ = n;
                if (camKind == 1) nearZ = 25.0f;
                if (camKind == 2) { vp[0] = INFINITY; vp[5] = -INFINITY; vp[10] = NAN; }
                if (camKind == 3) { vp[12] = vp[13] = vp[14] = vp[15] = 0.0f; }
                if (camKind == 4) { vp[15] = INFINITY; ivp[3] = NAN; }
                const size_t px = (size_t)W * H;
                uint32_t* depthBlock = static_cast<uint32_t*>(std::malloc(px * 4 + 4));
                uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4));
                uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4));
                uint8_t* ref = static_cast<uint8_t*>(std::malloc(px * 4));
                float* g[3];
                for (auto& p : g) p = static_cast<float*>(std::aligned_alloc(16, px * 16));
                const int shift = variant & 1;                             // planes at the block's start, or 4 bytes past it
                uint32_t* depth = depthBlock + shift;
                uint8_t* in = inBlock + 4 * shift;
                uint8_t* out = outBlock + 4 * shift;
                for (uint32_t y = 0; y < H; ++y)
                    for (uint32_t x = 0; x < W; ++x) {
                        const size_t i = (size_t)y * W + x;
                        // the ramp: a floor seen from above, 3 units deep at the bottom row and 60 at the top, every fifth column a post
                        const float z = 60.0f - 57.0f * (float)y / (float)(H > 1 ? H - 1 : 1) - ((x % 5u) == 0u ? 2.0f : 0.0f);
                        const uint32_t ramp = (uint32_t)((A + B / z) * 16777215.0f + 0.5f) | (rnd() << 24);
                        depth[i] = depthKind == 0 ? 0u : (depthKind == 1 ? 0xFFFFFFu : (depthKind == 2 ? rnd() : ramp));
                        for (int c = 0; c < 4; ++c) {
                            g[0][4 * i + c] = c == 3 ? unit() : 60.0f * unit() - 30.0f;
                            g[1][4 * i + c] = c == 3 && gKind == 1 ? 0.5f * unit() : unit();
                            g[2][4 * i + c] = gKind == 1 ? (c == 1 ? 1.0f : 0.1f * unit() - 0.05f) : 2.0f * unit() - 1.0f;
                        }
                        if (gKind == 2 && (x % 3u) == 0u) g[2][4 * i] = g[2][4 * i + 1] = g[2][4 * i + 2] = 0.0f;
                        if (gKind == 3) {
                            const float bad[4] = { NAN, INFINITY, -INFINITY, -1.0e38f };
                            const uint32_t r = rnd();
                            if ((r & 3u) != 3u) g[r & 3u][4 * i + ((r >> 2) & 3u)] = bad[(r >> 4) & 3u];
                        }
                    }
                for (size_t i = 0; i < px * 4; ++i) in[i] = (uint8_t)rnd();
                const uint32_t* gl = gloss[variant % 3];
                uint64_t plan[25];
                const uint32_t nEff = ssr_gloss_plan_ref(W, H, gl[1], plan);
                const size_t pyrBytes = (size_t)plan[24];
                uint8_t* pyr = block16(pyrBytes);
                uint8_t* pyrRef = block16(pyrBytes);
                std::memset(pyr, 0xA5, pyrBytes);
                std::memset(pyrRef, 0xA5, pyrBytes);
                ssr_gloss_pyramid_ref(in, W, H, gl[1], pyrRef);
                ssgh_pyramid(in, W, H, gl[1], pyr);
                ++calls;
                if (std::memcmp(pyr, pyrRef, pyrBytes) != 0) { std::fprintf(stderr, "the pyramids differ at %ux%u variant %d (%u levels built)\n", W, H, variant, nEff); return 1; }
                std::memset(ref, 0xA5, px * 4);
                ssr_gloss_ref(proj, vp, ivp, eye, &nearZ, g[0], g[1], g[2], depth, in, pyrRef, ref, W, H, 0, H, pr, gl, nullptr, nullptr);
                std::memset(out, 0xA5, px * 4);
                ssgh_glossy(proj, vp, ivp, eye, &nearZ, g[0], g[1], g[2], depth, in, pyr, out, W, H, 0, H, 0u, pr, gl);
                ++calls;
                if (std::memcmp(out, ref, px * 4) != 0) { std::fprintf(stderr, "the host body and the checker differ at %ux%u variant %d\n", W, H, variant); return 1; }
                // row ranges, odd starts and single rows included
                const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3 | 1u, H };
                std::memset(out, 0xA5, px * 4);
                for (int c = 0; c + 1 < 6; ++c) {
                    const uint32_t r0 = cuts[c] < H ? cuts[c] : H, r1 = cuts[c + 1] < H ? cuts[c + 1] : H;
                    if (r1 <= r0) continue;
                    ssgh_glossy(proj, vp, ivp, eye, &nearZ, g[0], g[1], g[2], depth, in, pyr, out, W, H, r0, r1 - r0, 0u, pr, gl);
                    ++calls;
                }
                if (std::memcmp(out, ref, px * 4) != 0) { std::fprintf(stderr, "stitched ranges differ at %ux%u variant %d\n", W, H, variant); return 1; }
                for (auto& p : g) std::free(p);
                std::free(pyr); std::free(pyrRef);
                std::free(depthBlock); std::free(inBlock); std::free(outBlock); std::free(ref);
            }
    std::printf("ssr gloss sanitizer run ok: %ld calls\n", calls);
    return 0;
}
