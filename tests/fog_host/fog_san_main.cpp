// fog_san_main.cpp -- a stand-alone program over fog_host.cpp for an ASan + UBSan run of the kernel body (TEST INFRASTRUCTURE):
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -I crychic_renderer_amd/csrc tests/fog_host/fog_san_main.cpp tests/fog_host/fog_host.cpp -o /tmp/fog_san && /tmp/fog_san
// Every plane and every map is a heap block of exactly its size (the planes also 4 bytes past the block's start), so a read or a write
// outside one is reported.  The corpus's frame sizes, map sides, step counts and parameter sets over depth planes of 0, of 0xFFFFFF
// and of noise and maps of 0, of 0xFFFFFF, of noise and the half-plane step, under a camera built here (an eye at (0, 2, -15) looking
// along +z, four nested cascades seen from straight above); the same with the eye far outside the cascades and with non-finite
// entries in InvViewProj.  Whole frames out of place and in place, and row ranges, must agree.  Prints the number of calls; exits
// non-zero on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" uint32_t fgh_fog(const float* invViewProj, const float* eye, const float* shadowTransforms, const uint32_t* depth,
                            const uint32_t* const* maps, uint32_t dim, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                            uint32_t rows, const uint32_t* params);

static uint32_t g_seed = 2024u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }
static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 5 }, { 63, 4 }, { 64, 4 }, { 65, 7 }, { 130, 9 }, { 322, 190 } };
    const uint32_t dims[] = { 1, 17, 100, 256 };
    // density, maxDistance, steps, ambient, sun
    const uint32_t params[][9] = { { fbits(0.02f), fbits(100.0f), 16, 70, 80, 100, 150, 140, 110 }, { fbits(4e-6f), fbits(40.0f), 1, 70, 80, 100, 150, 140, 110 },
                                   { fbits(0.01f), fbits(150.0f), 2, 70, 80, 100, 150, 140, 110 }, { fbits(0.1f), fbits(60.0f), 63, 255, 255, 255, 255, 250, 255 },
                                   { fbits(16.0f), fbits(100.0f), 64, 70, 80, 100, 150, 140, 110 }, { fbits(0.0f), fbits(100.0f), 16, 70, 80, 100, 150, 140, 110 } };
    long calls = 0;
    int variant = 0;
    for (const auto& sz : sizes)
        for (uint32_t dim : dims)
            for (const auto& pr : params) {
                const uint32_t W = sz[0], H = sz[1];
                ++variant;
                if (W * H > 10000u && (variant % 3) != 0) continue;         // the large frame: every third combination
                const int depthKind = variant % 3, mapKind = (variant / 3) % 4, camKind = (variant / 12) % 4;
                // the camera: InvViewProj stored transposed (column c of the row-vector matrix at floats 4c ..)
                const float n = 1.0f, f = 100.0f, tanv = 0.41421356f, aspect = (float)W / (float)H;
                float eye[3] = { 0.0f, 2.0f, -15.0f };
                const float wz = -(f - n) / (n * f), ww = 1.0f / n;
                float ivp[16] = { aspect * tanv, 0, eye[0] * wz, eye[0] * ww,  0, tanv, eye[1] * wz, eye[1] * ww,  0, 0, eye[2] * wz, 1.0f + eye[2] * ww,  0, 0, wz, ww };
                if (camKind == 1) { eye[0] = 1.0e4f; eye[1] = 1.0e4f; eye[2] = -1.0e4f; }
                if (camKind == 2) { ivp[0] = INFINITY; ivp[5] = -INFINITY; ivp[10] = NAN; }
                if (camKind == 3) { ivp[12] = ivp[13] = ivp[14] = ivp[15] = 0.0f; }
                float st[4][16];
                const float extent[4] = { 40.0f, 70.0f, 110.0f, 160.0f };
                for (int j = 0; j < 4; ++j) {
                    const float s = 1.0f / extent[j];
                    const float m[16] = { s, 0, 0, 0.5f,  0, 0, s, 0.5f,  0, -0.02f, 0, 0.5f,  0, 0, 0, 1 };
                    std::memcpy(st[j], m, sizeof m);
                }
                const size_t px = (size_t)W * H;
                uint32_t* depthBlock = static_cast<uint32_t*>(std::malloc(px * 4 + 4));
                uint8_t* inBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4));
                uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(px * 4 + 4));
                uint8_t* ref = static_cast<uint8_t*>(std::malloc(px * 4));
                const int shift = variant & 1;                             // planes at the block's start, or 4 bytes past it
                uint32_t* depth = depthBlock + shift;
                uint8_t* in = inBlock + 4 * shift;
                uint8_t* out = outBlock + 4 * shift;
                for (size_t i = 0; i < px; ++i) depth[i] = depthKind == 0 ? 0u : (depthKind == 1 ? 0xFFFFFFu : rnd());
                for (size_t i = 0; i < px * 4; ++i) in[i] = (uint8_t)rnd();
                uint32_t* maps[4];
                for (int j = 0; j < 4; ++j) {
                    maps[j] = static_cast<uint32_t*>(std::malloc((size_t)dim * dim * 4));
                    for (uint32_t y = 0; y < dim; ++y)
                        for (uint32_t x = 0; x < dim; ++x)
                            maps[j][(size_t)y * dim + x] = mapKind == 0 ? 0u : (mapKind == 1 ? 0xFFFFFFu : (mapKind == 2 ? rnd() : (x >= dim / 2 ? 0xFFFFFFu : 0u)));
                }
                std::memset(ref, 0xA5, px * 4);
                fgh_fog(ivp, eye, &st[0][0], depth, maps, dim, in, ref, W, H, 0, H, pr);
                ++calls;
                // row ranges, odd starts and single rows included
                const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3 | 1u, H };
                std::memset(out, 0xA5, px * 4);
                for (int c = 0; c + 1 < 6; ++c) {
                    const uint32_t r0 = cuts[c] < H ? cuts[c] : H, r1 = cuts[c + 1] < H ? cuts[c + 1] : H;
                    if (r1 <= r0) continue;
                    fgh_fog(ivp, eye, &st[0][0], depth, maps, dim, in, out, W, H, r0, r1 - r0, pr);
                    ++calls;
                }
                if (std::memcmp(out, ref, px * 4) != 0) { std::fprintf(stderr, "stitched ranges differ at %ux%u variant %d\n", W, H, variant); return 1; }
                // in place
                std::memcpy(out, in, px * 4);
                fgh_fog(ivp, eye, &st[0][0], depth, maps, dim, out, out, W, H, 0, H, pr);
                ++calls;
                if (std::memcmp(out, ref, px * 4) != 0) { std::fprintf(stderr, "in place differs at %ux%u variant %d\n", W, H, variant); return 1; }
                if (pr[0] == 0u && std::memcmp(ref, in, px * 4) != 0) { std::fprintf(stderr, "density 0 is not a copy at %ux%u\n", W, H); return 1; }
                for (int j = 0; j < 4; ++j) std::free(maps[j]);
                std::free(depthBlock); std::free(inBlock); std::free(outBlock); std::free(ref);
            }
    std::printf("fog sanitizer run ok: %ld calls\n", calls);
    return 0;
}
