// decal_san_main.cpp -- a stand-alone program over decal_host.cpp for an ASan + UBSan run of the kernel body (TEST INFRASTRUCTURE):
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I crychic_renderer_amd/csrc tests/decal_host/decal_san_main.cpp tests/decal_host/decal_host.cpp \
//       -L crychic_renderer_amd -lcrychic_hip -Wl,-rpath,$PWD/crychic_renderer_amd -o /tmp/decal_san && /tmp/decal_san
// (the library only for crychic_decal_from_box, pure host code)
// Every plane, the decal array and every texture chain is a heap block of exactly its size, so a read or a write outside one is
// reported.  The corpus's frame sizes under the three format mixes, 0, 1, 63 and 64 random decals (random affine boxes, bounds of all
// space or a random box, every flag combination, texture indices in and out of range) over chains of 1 x 1, 2 x 2, 5 x 3 (three
// levels) and 16 x 16 (five levels) texels, positions with NaN and infinities; whole frames and row ranges must agree.  Prints the
// number of calls; exits non-zero on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "crychic_hip.h"

extern "C" uint32_t dch_apply(const float* view, const float* proj, const uint32_t* depth, void* g0, void* g1, void* g2, uint32_t formatFlags,
                              const crychic_decal* decals, uint32_t nDecals, const crychic_texture* textures, uint32_t nTextures, uint32_t W,
                              uint32_t H, uint32_t row0, uint32_t rows, uint64_t* masks);

static uint32_t g_seed = 2026u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed ^ (g_seed >> 15); }
static float unit() { return (float)(rnd() & 0xFFFFFFu) / 16777216.0f; }
static float range(float a, float b) { return a + (b - a) * unit(); }

static uint16_t to_half(float f) { _Float16 h = (_Float16)f; uint16_t u; std::memcpy(&u, &h, 2); return u; }

int main()
{
    const uint32_t sizes[][2] = { { 1, 1 }, { 3, 5 }, { 63, 4 }, { 64, 4 }, { 65, 7 }, { 130, 9 } };
    const uint32_t counts[] = { 0, 1, 63, 64 };
    const uint32_t mixes[] = { 0u, 0x6000u, 0x7000u };
    const uint32_t shapes[][3] = { { 1, 1, 1 }, { 2, 2, 1 }, { 5, 3, 3 }, { 16, 16, 5 } };
    long calls = 0;
    int variant = 0;
    for (const auto& sz : sizes)
        for (uint32_t n : counts)
            for (uint32_t mix : mixes) {
                const uint32_t W = sz[0], H = sz[1];
                ++variant;
                const size_t px = (size_t)W * H;
                float view[16] = { 0 }, proj[16] = { 0 };
                view[10] = 1.0f; view[11] = 15.0f;
                proj[5] = (variant & 1) ? 2.4142f : 0.05f;
                // textures: exact-size chains
                crychic_texture tex[4];
                for (int t = 0; t < 4; ++t) {
                    size_t texels = 0;
                    for (uint32_t k = 0, w = shapes[t][0], h = shapes[t][1]; k < shapes[t][2]; ++k, w = w > 1 ? w >> 1 : 1, h = h > 1 ? h >> 1 : 1) texels += (size_t)w * h;
                    uint8_t* p = static_cast<uint8_t*>(std::malloc(texels * 4));
                    for (size_t i = 0; i < texels * 4; ++i) p[i] = (uint8_t)rnd();
                    tex[t] = crychic_texture{ p, shapes[t][0], shapes[t][1], shapes[t][2] };
                }
                crychic_decal* decals = static_cast<crychic_decal*>(std::malloc((size_t)(n ? n : 1) * sizeof(crychic_decal)));
                for (uint32_t d = 0; d < n; ++d) {
                    float world[16] = { 0 };
                    for (int r = 0; r < 3; ++r) {
                        for (int a = 0; a < 3; ++a) world[4 * r + a] = range(-3.0f, 3.0f) + (r == a ? 4.0f : 0.0f);
                        world[4 * r + 3] = range(-3.0f, 3.0f);
                    }
                    world[15] = 1.0f;
                    const uint32_t t = rnd() % 4u;
                    if (crychic_decal_from_box(world, shapes[t][0], shapes[t][1], 0.8f, -0.3f, &decals[d]) != 0) { std::fprintf(stderr, "decal_from_box refused\n"); return 1; }
                    decals[d].texture = (rnd() % 10u == 0) ? 4u + rnd() % 3u : t;
                    decals[d].normalTexture = (rnd() % 3u == 0) ? CRYCHIC_DECAL_NO_TEXTURE : rnd() % 5u;
                    decals[d].flags = rnd() % 16u;
                    decals[d].opacity = unit();
                    if (rnd() % 4u == 0) for (int c = 0; c < 3; ++c) { decals[d].boundsMin[c] = -INFINITY; decals[d].boundsMax[c] = INFINITY; }
                    if (rnd() % 8u == 0) decals[d].texelsPerUnit *= (rnd() & 1u) ? 1.0e-3f : 1.0e3f;
                }
                uint32_t* depth = static_cast<uint32_t*>(std::malloc(px * 4));
                for (size_t i = 0; i < px; ++i) depth[i] = (rnd() % 4u == 0) ? (rnd() | 0xFFFFFFu) : rnd();
                const size_t bytes[3] = { px * ((mix & 0x1000u) ? 8u : 16u), px * ((mix & 0x2000u) ? 8u : 16u), px * ((mix & 0x4000u) ? 8u : 16u) };
                void *src[3], *whole[3], *parts[3];
                for (int k = 0; k < 3; ++k) {
                    src[k] = std::malloc(bytes[k]); whole[k] = std::malloc(bytes[k]); parts[k] = std::malloc(bytes[k]);
                    for (size_t i = 0; i < px * 4; ++i) {
                        float v = k == 0 ? range(-4.0f, 4.0f) : (k == 1 ? unit() : range(-1.0f, 1.0f));
                        if (k == 0 && (i & 3) != 3 && rnd() % 50u == 0) v = (rnd() & 1u) ? NAN : ((rnd() & 1u) ? INFINITY : -INFINITY);
                        if (bytes[k] == px * 8) static_cast<uint16_t*>(src[k])[i] = to_half(v);
                        else static_cast<float*>(src[k])[i] = v;
                    }
                    std::memcpy(whole[k], src[k], bytes[k]);
                    std::memcpy(parts[k], src[k], bytes[k]);
                }
                dch_apply(view, proj, depth, whole[0], whole[1], whole[2], mix, n ? decals : nullptr, n, tex, 4, W, H, 0, H, nullptr);
                ++calls;
                const uint32_t cuts[] = { 0, 1, H / 3, H / 3 + 1, (2 * H) / 3 | 1u, H };
                uint32_t done = 0;                                         // rows [0, done) are decaled: a row taken twice would stack
                for (int c = 1; c < 6; ++c) {
                    const uint32_t r1 = cuts[c] < H ? cuts[c] : H;
                    if (r1 <= done) continue;
                    dch_apply(view, proj, depth, parts[0], parts[1], parts[2], mix, n ? decals : nullptr, n, tex, 4, W, H, done, r1 - done, nullptr);
                    done = r1;
                    ++calls;
                }
                for (int k = 0; k < 3; ++k) {
                    if (std::memcmp(whole[k], parts[k], bytes[k]) != 0) { std::fprintf(stderr, "stitched ranges differ at %ux%u variant %d plane %d\n", W, H, variant, k); return 1; }
                    if (n == 0 && std::memcmp(whole[k], src[k], bytes[k]) != 0) { std::fprintf(stderr, "no decals changed plane %d\n", k); return 1; }
                    std::free(src[k]); std::free(whole[k]); std::free(parts[k]);
                }
                std::free(depth); std::free(decals);
                for (int t = 0; t < 4; ++t) std::free(const_cast<uint8_t*>(tex[t].rgba8_dev));
            }
    std::printf("decal sanitizer run ok: %ld calls\n", calls);
    return 0;
}
