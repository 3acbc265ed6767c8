// sky_san_main.cpp -- a stand-alone program over sky_host.cpp and the checker for an ASan + UBSan run of both (TEST INFRASTRUCTURE):
//   clang -O1 -g -std=c99 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -c tests/sky_ref/sky_ref.c -o /tmp/sky_ref.o
//   clang++ -O1 -g -std=c++17 -ffp-contract=off -mfma -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
//       -I crychic_renderer_amd/csrc tests/sky_host/sky_san_main.cpp tests/sky_host/sky_host.cpp /tmp/sky_ref.o -lm -o /tmp/sky_san && /tmp/sky_san
// The dim 8 cases of the corpus (tests/sky_lib.py): the seven suns under the three step counts and both altitudes, the wide disc and
// the two parameter sets off the defaults.  Every cube is a heap block of exactly its size (every other one 4 bytes past the block's
// start), so a write outside one is reported.  The host build of the kernel body and the checker must agree in every byte, whole
// cubes and every split of the six faces into two calls, and on the sun's colour bit for bit.  Prints the number of calls; exits
// non-zero on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Params {
    float sunDir[3], altitude, sunIntensity, exposure, sunAngularRadius, groundAlbedo;
    uint32_t viewSteps, sunSteps, reserved[2];
};

extern "C" uint32_t skh_render_sky(uint8_t* cube, uint32_t dim, uint32_t face0, uint32_t faces, const void* params);
extern "C" void skh_sun_colour(const void* params, float* rgb);
extern "C" void sky_ref(uint32_t* cube, uint32_t dim, uint32_t face0, uint32_t faces, const void* params, uint64_t* counters);
extern "C" void sky_ref_sun_colour(const void* params, float* rgb);

static Params defaults()
{
    Params p = {};
    p.sunDir[1] = 0.5f; p.sunDir[2] = -0.8660254f;
    p.altitude = 0.002f; p.sunIntensity = 20.0f; p.exposure = 2.0f; p.sunAngularRadius = 0.02f; p.groundAlbedo = 0.3f;
    p.viewSteps = 16u; p.sunSteps = 8u;
    return p;
}

int main()
{
    const uint32_t dim = 8u;
    const size_t bytes = (size_t)6 * dim * dim * 4;
    const double deg = 3.14159265358979323846 / 180.0;
    const double elevations[] = { 90.0, 30.0, 5.0, 0.0, -3.0, -30.0 };
    const uint32_t steps[][2] = { { 1u, 1u }, { 16u, 8u }, { 64u, 32u } };
    const float altitudes[] = { 0.0f, 50.0f };
    Params cases[64];
    int n = 0;
    for (int s = 0; s < 7; ++s)
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 2; ++a) {
                if ((s + k + a) % 2) continue;          // half of the cross product: every sun meets every step count and both altitudes
                Params p = defaults();
                if (s < 6) { p.sunDir[0] = 0.0f; p.sunDir[1] = (float)std::sin(elevations[s] * deg); p.sunDir[2] = (float)-std::cos(elevations[s] * deg); }
                else { p.sunDir[0] = 0.3f; p.sunDir[1] = 0.5f; p.sunDir[2] = -0.8f; }
                p.viewSteps = steps[k][0]; p.sunSteps = steps[k][1]; p.altitude = altitudes[a];
                cases[n++] = p;
            }
    { Params p = defaults(); p.sunAngularRadius = 0.3f; cases[n++] = p; }       // at dim 8 a texel spans a quarter radian
    { Params p = defaults(); p.sunDir[0] = 0.0f; p.sunDir[1] = 87.0f; p.sunDir[2] = -996.0f; p.sunIntensity = 400.0f; p.exposure = 0.5f;
      p.groundAlbedo = 1.0f; p.altitude = 3.0f; p.viewSteps = 5u; p.sunSteps = 3u; cases[n++] = p; }
    { Params p = defaults(); p.groundAlbedo = 0.0f; p.sunAngularRadius = 0.0f; p.viewSteps = 7u; p.sunSteps = 31u; cases[n++] = p; }
    long calls = 0;
    for (int c = 0; c < n; ++c) {
        const Params& p = cases[c];
        const int shift = c & 1;                        // the cube at the block's start, or 4 bytes past it
        uint8_t* refBlock = static_cast<uint8_t*>(std::malloc(bytes + 4));
        uint8_t* outBlock = static_cast<uint8_t*>(std::malloc(bytes + 4));
        uint8_t* ref = refBlock + 4 * shift;
        uint8_t* out = outBlock + 4 * shift;
        std::memset(ref, 0xA5, bytes);
        sky_ref(reinterpret_cast<uint32_t*>(ref), dim, 0, 6, &p, nullptr);
        std::memset(out, 0xA5, bytes);
        skh_render_sky(out, dim, 0, 6, &p);
        calls += 2;
        if (std::memcmp(out, ref, bytes) != 0) { std::fprintf(stderr, "the host body and the checker differ in case %d\n", c); return 1; }
        for (uint32_t k = 0; k <= 6; ++k) {
            std::memset(out, 0xA5, bytes);
            skh_render_sky(out, dim, 0, k, &p);
            skh_render_sky(out, dim, k, 6 - k, &p);
            calls += 2;
            if (std::memcmp(out, ref, bytes) != 0) { std::fprintf(stderr, "faces [0,%u) + [%u,6) differ in case %d\n", k, k, c); return 1; }
        }
        float a[3], b[3];
        skh_sun_colour(&p, a);
        sky_ref_sun_colour(&p, b);
        calls += 2;
        if (std::memcmp(a, b, sizeof a) != 0) { std::fprintf(stderr, "the sun colours differ in case %d\n", c); return 1; }
        std::free(refBlock); std::free(outBlock);
    }
    std::printf("sky sanitizer run ok: %d cases, %ld calls\n", n, calls);
    return 0;
}
