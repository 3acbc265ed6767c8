// parallax_host.cpp -- the box-projected reflection lookup built for the host (TEST INFRASTRUCTURE): light_core.hpp's probe_project
// and the CubeGlossBox instantiations of light_pixel, the bodies of the parallax variants of light_general.hip, bound through
// light_bind.hpp as the library binds them; and light_bind.hpp's checks of the flag and of the setter's arguments.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "host_light_probe.hpp"

// The correction of one (p, r) under the twelve floats of a probe volume, through probe_load and probe_project.
extern "C" void xh_correct(const float* p, const float* r, const float* probe, float* out)
{
    using namespace cry;
    const f3 d = probe_project(probe_load(probe), f3{ p[0], p[1], p[2] }, f3{ r[0], r[1], r[2] });
    out[0] = d.x; out[1] = d.y; out[2] = d.z;
}

// `count` of them: p, r (count x 3) and probe (count x 12) to out (count x 3).
extern "C" void xh_correct_many(const float* p, const float* r, const float* probe, float* out, size_t count)
{
    for (size_t i = 0; i < count; ++i) xh_correct(p + 3 * i, r + 3 * i, probe + 12 * i, out + 3 * i);
}

extern "C" uint64_t xh_probe_offset(uint32_t dim, uint32_t levels) { return cry::parallax_probe_offset(dim, levels); }

// The binding's validation of a call with the flag: 0 ok, 1 no gloss chain, 2 null cube map, 3 misaligned probe volume.
extern "C" int xh_check(uint32_t flags, uintptr_t cube, uint32_t cubeDim)
{
    return (int)cry::parallax_check(flags, reinterpret_cast<const void*>(cube), cubeDim);
}

// The message the entries report that refusal with, formatted as they format it.
extern "C" int xh_check_message(uint32_t flags, uintptr_t cube, uint32_t cubeDim, char* out, size_t cap)
{
    const cry::ParallaxCheck c = cry::parallax_check(flags, reinterpret_cast<const void*>(cube), cubeDim);
    return std::snprintf(out, cap, cry::parallax_check_message(c), cry::parallax_probe_offset(cubeDim, (flags >> 16) & 15u));
}

// crychic_set_cube_probe_volume's check of its values: 1 valid.
extern "C" int xh_volume_valid(const float* pos, const float* boxMin, const float* boxMax) { return cry::probe_volume_valid(pos, boxMin, boxMax) ? 1 : 0; }

// What tests/hostsim/host_light.hpp's three-policy visit answers for the flags: 1 served (one of today's seven combinations), 0 not.
extern "C" int xh_old_visit(uint32_t flags)
{
    int calls = 0;
    const bool served = cry::light_variant_visit(cry::light_variant(flags, (flags >> 16) & 15u), [&](auto, auto, auto) { ++calls; });
    return served ? calls : 0;
}

// Every crychic_deferred_light* entry on the host, with or without CRYCHIC_LIGHT_CUBE_PARALLAX: the checks api.cpp makes, then
// host_light_probe.  -1: refused.
extern "C" int xh_light(const crychic_pass_constants* cb, const void* g0, const void* g1, const void* g2,
                        const uint32_t* depth, const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                        const uint8_t* cube, uint32_t cubeDim, uint8_t* out, float* radiance, uint32_t W, uint32_t H,
                        uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                        const crychic_light* pointLights, uint32_t numPointLights, const crychic_light* spotLights,
                        uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim, const uint32_t* const* shadowMaps,
                        uint32_t pointShadowCount, uint32_t pointShadowDim, const uint32_t* const* pointMaps, const float* shadowProj)
{
    using namespace cry;
    if (ambient_sh_check(flags, cube, cubeDim) != AmbientShCheck::Ok || env_brdf_check(flags, cube, cubeDim) != EnvBrdfCheck::Ok ||
        parallax_check(flags, cube, cubeDim) != ParallaxCheck::Ok) return -1;
    return host_light_probe(cb, g0, g1, g2, depth, ambient, shadow, shadowDim, cube, cubeDim, out, radiance, W, H, row0, rows, numDirLights,
                            pcfSearchRadius, flags, pointLights, numPointLights, spotLights, numSpotLights, shadowCount, shadowMapDim, shadowMaps,
                            pointShadowCount, pointShadowDim, pointMaps, shadowProj) ? 0 : -1;
}
