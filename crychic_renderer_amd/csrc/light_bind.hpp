// light_bind.hpp -- host side of one lighting call: what the kernels take by value (LightParams, SpotShadows, PointShadows) from the
// caller's arguments, and which kernel family and instantiation serve the call.  Plain C++: no HIP runtime call, nothing that can fail -- api.cpp
// validates first and reports; the host build of the kernel bodies (tests/hostsim) binds through the same functions, so the CPU
// tier executes the binding the library ships.
#pragma once
#include <cstring>
#include "light_core.hpp"

namespace cry {

// The frame's constants and the four cascades into P, with everything the kernels expect precomputed on the host.  Leaves
// P.pointLights / P.numPointLights alone (bind_point_lights).
inline void bind_light_params(LightParams& P, const crychic_pass_constants& cb, const uint32_t* const shadow[4], uint32_t shadowDim,
                              uint32_t cubeDim, uint32_t W, uint32_t H, int numDirLights, float pcfSearchRadius, uint32_t flags)
{
    std::memcpy(P.ViewProjTex, cb.ViewProjTex, sizeof P.ViewProjTex);
    std::memcpy(P.ShadowTransforms, cb.ShadowTransforms, sizeof P.ShadowTransforms);  // cascades 0..3
    std::memcpy(P.InvProj, cb.InvProj, sizeof P.InvProj);
    std::memcpy(P.InvView, cb.InvView, sizeof P.InvView);
    std::memcpy(P.EyePosW, cb.EyePosW, sizeof P.EyePosW);
    P.pcfSearchRadius = pcfSearchRadius;
    std::memcpy(P.AmbientLight, cb.AmbientLight, sizeof P.AmbientLight);
    std::memcpy(P.Lights, cb.Lights, sizeof P.Lights);
    for (int i = 0; i < 4; ++i) P.shadow[i] = shadow[i];
    P.shadowDim = shadowDim;
    P.cubeDim = cubeDim;
    P.W = W;
    P.H = H;
    P.numDirLights = numDirLights;
    P.flags = flags;
    // CRYCHIC_LIGHT_CUBE_LEVELS: the cube map's mip chain (0 / 1 = level 0 alone); a chain ends at 1 x 1 at the latest
    P.cubeLevels = (flags >> 16) & 15u;
    P.shadowWIsOne = light_shadow_w_is_one(P.ShadowTransforms) ? 1u : 0u;
    P.darkLights = light_dark_mask(P.Lights, numDirLights);
    P.unitLights = light_dark_lengths_ok(P.Lights, numDirLights) ? 1u : 0u;
    P.rcpW = rcp((float)W);          // sky_pixel's pixel-centre uv: (x + 0.5) * rcp(W), the reciprocal taken once
    P.rcpH = rcp((float)H);
    light_params_derive(P);
}

// The point lights of the pass (a device buffer when there are any).  Touches none of P's other fields.
inline void bind_point_lights(LightParams& P, const crychic_light* points, uint32_t nPoints)
{
    P.pointLights = points;
    P.numPointLights = nPoints;
}

// The first `count` spot shadow maps and cb.ShadowTransforms[4 + k] into S.  count 0 leaves S zeroed (S.count = 0): the kernels
// without spot shadows.
inline void bind_spot_shadows(SpotShadows& S, const crychic_pass_constants& cb, const uint32_t* const* maps, uint32_t count, uint32_t dim)
{
    std::memset(&S, 0, sizeof S);
    if (count == 0) return;
    for (uint32_t k = 0; k < count; ++k) {
        S.maps[k] = maps[k];
        std::memcpy(S.T[k], cb.ShadowTransforms[4 + k], sizeof S.T[k]);
    }
    S.count = count;
    S.dim = dim;
    S.dx = 1.0f / (float)dim;                          // IEEE division on the host: correctly rounded
}

// The first `count` cube shadow maps and their projections into PS.  shadowProj: 16 floats per light, untransposed
// (crychic_update_point_shadow_transforms).  count 0 leaves PS zeroed: the kernels without point shadows.
inline void bind_point_shadows(PointShadows& PS, const uint32_t* const* maps, const float* shadowProj, uint32_t count, uint32_t dim)
{
    std::memset(&PS, 0, sizeof PS);
    if (count == 0) return;
    for (uint32_t k = 0; k < count; ++k) {
        PS.maps[k] = maps[k];
        for (int i = 0; i < 4; ++i)                        // transposed: row i of M = column i of shadowProj (as the spot T)
            for (int j = 0; j < 4; ++j) PS.M[k][4 * i + j] = shadowProj[16 * k + 4 * j + i];
    }
    PS.count = count;
    PS.dim = dim;
    PS.dx = 1.0f / (float)dim;                         // IEEE division on the host: correctly rounded
}

// CRYCHIC_LIGHT_AMBIENT_SH: what a call with the flag must satisfy before it is bound (api.cpp turns the answer into its error).
enum class AmbientShCheck { Ok, DerivativeChain, NullCube, MisalignedTail };
// Byte offset of the environment tail behind a cube map of `levels` levels (crychic_cube_sh_offset): the chain rounded up to 16.
inline size_t ambient_sh_offset(uint32_t cubeDim, uint32_t levels)
{
    size_t n = 0;
    for (uint32_t k = 0; k < (levels ? levels : 1u); ++k) { const size_t d = cube_level_dim(cubeDim, k); n += 6u * d * d * 4u; }
    return (n + 15u) & ~(size_t)15u;
}
inline AmbientShCheck ambient_sh_check(uint32_t flags, const void* cube, uint32_t cubeDim)
{
    if (!(flags & CRYCHIC_LIGHT_AMBIENT_SH)) return AmbientShCheck::Ok;
    const uint32_t levels = (flags >> 16) & 15u;
    if (levels > 1u && !(flags & CRYCHIC_LIGHT_CUBE_GLOSS)) return AmbientShCheck::DerivativeChain;
    if (!cube) return AmbientShCheck::NullCube;
    if ((reinterpret_cast<uintptr_t>(cube) + ambient_sh_offset(cubeDim, levels)) & 3u) return AmbientShCheck::MisalignedTail;
    return AmbientShCheck::Ok;
}

// CRYCHIC_LIGHT_ENV_BRDF: the same for the split-sum weight of the reflection.  The table follows the environment tail.
enum class EnvBrdfCheck { Ok, NeedsGlossChain, NullCube, MisalignedTable };
inline size_t env_brdf_offset(uint32_t cubeDim, uint32_t levels) { return ambient_sh_offset(cubeDim, levels) + CRYCHIC_CUBE_SH_BYTES; }
inline EnvBrdfCheck env_brdf_check(uint32_t flags, const void* cube, uint32_t cubeDim)
{
    if (!(flags & CRYCHIC_LIGHT_ENV_BRDF)) return EnvBrdfCheck::Ok;
    const uint32_t levels = (flags >> 16) & 15u;
    if (levels < 2u || !(flags & CRYCHIC_LIGHT_CUBE_GLOSS)) return EnvBrdfCheck::NeedsGlossChain;
    if (!cube) return EnvBrdfCheck::NullCube;
    if ((reinterpret_cast<uintptr_t>(cube) + env_brdf_offset(cubeDim, levels)) & 3u) return EnvBrdfCheck::MisalignedTable;
    return EnvBrdfCheck::Ok;
}
// The message api.cpp reports a refusal with (a printf format; MisalignedTable takes the table's offset as %zu), here so that the
// host harness states the same text.
inline const char* env_brdf_check_message(EnvBrdfCheck c)
{
    switch (c) {
    case EnvBrdfCheck::NeedsGlossChain:
        return "CRYCHIC_LIGHT_ENV_BRDF needs a prefiltered chain: CRYCHIC_LIGHT_CUBE_LEVELS(n) with n > 1 and CRYCHIC_LIGHT_CUBE_GLOSS";
    case EnvBrdfCheck::NullCube: return "CRYCHIC_LIGHT_ENV_BRDF: null cube map";
    case EnvBrdfCheck::MisalignedTable: return "CRYCHIC_LIGHT_ENV_BRDF: the table at cube_dev + %zu is not 4-byte aligned";
    default: return "";
    }
}

// CRYCHIC_LIGHT_CUBE_PARALLAX: the same for the box-projected reflection lookup.  The probe volume sits in the environment tail.
enum class ParallaxCheck { Ok, NeedsGlossChain, NullCube, MisalignedProbe };
inline size_t parallax_probe_offset(uint32_t cubeDim, uint32_t levels) { return ambient_sh_offset(cubeDim, levels) + CRYCHIC_CUBE_PROBE_OFFSET; }
inline ParallaxCheck parallax_check(uint32_t flags, const void* cube, uint32_t cubeDim)
{
    if (!(flags & CRYCHIC_LIGHT_CUBE_PARALLAX)) return ParallaxCheck::Ok;
    const uint32_t levels = (flags >> 16) & 15u;
    if (levels < 2u || !(flags & CRYCHIC_LIGHT_CUBE_GLOSS)) return ParallaxCheck::NeedsGlossChain;
    if (!cube) return ParallaxCheck::NullCube;
    if ((reinterpret_cast<uintptr_t>(cube) + parallax_probe_offset(cubeDim, levels)) & 3u) return ParallaxCheck::MisalignedProbe;
    return ParallaxCheck::Ok;
}
// The message of a refusal (a printf format; MisalignedProbe takes the probe volume's offset as %zu), shared with the host harness.
inline const char* parallax_check_message(ParallaxCheck c)
{
    switch (c) {
    case ParallaxCheck::NeedsGlossChain:
        return "CRYCHIC_LIGHT_CUBE_PARALLAX needs a prefiltered chain: CRYCHIC_LIGHT_CUBE_LEVELS(n) with n > 1 and CRYCHIC_LIGHT_CUBE_GLOSS";
    case ParallaxCheck::NullCube: return "CRYCHIC_LIGHT_CUBE_PARALLAX: null cube map";
    case ParallaxCheck::MisalignedProbe: return "CRYCHIC_LIGHT_CUBE_PARALLAX: the probe volume at cube_dev + %zu is not 4-byte aligned";
    default: return "";
    }
}
// crychic_set_cube_probe_volume's arguments: finite, and boxMin < pos < boxMax strictly in every component (a NaN fails).
inline bool probe_volume_valid(const float pos[3], const float boxMin[3], const float boxMax[3])
{
    const float inf = __builtin_inff();
    for (int k = 0; k < 3; ++k)
        if (!(__builtin_fabsf(boxMin[k]) < inf && __builtin_fabsf(boxMax[k]) < inf && boxMin[k] < pos[k] && pos[k] < boxMax[k])) return false;
    return true;
}

// ---- which kernels serve a lighting call -------------------------------------------------------------------------
// One family per set of kernel arguments; ZERO_RADIUS and the LightVariant below select the instantiation inside every family.
enum class LightFamily {
    Frame,            // light_kernel<z, false>: no local light, no CRYCHIC_FIX_* bit, no chain -- the reference as written
    FrameFix,         // light_kernel<z, true, mips>: FIX compiled in (the chain is not the benchmark's instantiation)
    Points,           // light_points_kernel
    Spots,            // light_spots_kernel: point lights, then spot lights
    SpotsShadowed,    // light_spots_shadowed_kernel: SpotShadowOf on the spot lights
    PointShadows,     // light_point_shadows_kernel: PointShadowOf on the point lights, and the spot lights with SpotShadowOf even at a
                      // spot shadow count of 0 (factor 1)
    // The general family (light_general.hip): every call with a half4 plane (CRYCHIC_GBUFFER_G*_F16),
    // CRYCHIC_LIGHT_CUBE_GLOSS, CRYCHIC_LIGHT_AMBIENT_SH or CRYCHIC_LIGHT_ENV_BRDF (CRYCHIC_LIGHT_CUBE_PARALLAX comes with the gloss
    // flag).  Planes of any format mix and FIX compiled in;
    // the LightVariant below picks the instantiation.
    FormatsFrame,     // light_general_kernel: no local light
    FormatsLocal,     // light_general_local_kernel: local lights of whatever kind; both shadow functors whatever the counts
};
inline LightFamily light_family(uint32_t flags, uint32_t numPointLights, uint32_t numSpots, uint32_t spotShadowCount,
                                uint32_t pointShadowCount, uint32_t cubeLevels)
{
    if (flags & (CRYCHIC_GBUFFER_F16_MASK | CRYCHIC_LIGHT_CUBE_GLOSS | CRYCHIC_LIGHT_AMBIENT_SH | CRYCHIC_LIGHT_ENV_BRDF)) return (numPointLights || numSpots) ? LightFamily::FormatsLocal : LightFamily::FormatsFrame;
    if (pointShadowCount) return LightFamily::PointShadows;
    if (numSpots && spotShadowCount) return LightFamily::SpotsShadowed;
    if (numSpots) return LightFamily::Spots;
    if (numPointLights) return LightFamily::Points;
    const bool fix = (flags & (CRYCHIC_FIX_Q1 | CRYCHIC_FIX_Q3 | CRYCHIC_FIX_Q4)) != 0;
    return (cubeLevels > 1u || fix) ? LightFamily::FrameFix : LightFamily::Frame;
}
// What a family's kernels compile in: every family but Frame instantiates light_pixel with FIX; the local families walk lights
// (light_local_tile); SHADOWED / POINT_SHADOWED of light_local_tile.
constexpr bool light_family_fix(LightFamily f) { return f != LightFamily::Frame; }
constexpr bool light_family_local(LightFamily f)
{
    return f != LightFamily::Frame && f != LightFamily::FrameFix && f != LightFamily::FormatsFrame;
}
constexpr bool light_family_spot_shadows(LightFamily f)
{
    return f == LightFamily::SpotsShadowed || f == LightFamily::PointShadows || f == LightFamily::FormatsLocal;
}
constexpr bool light_family_point_shadows(LightFamily f) { return f == LightFamily::PointShadows || f == LightFamily::FormatsLocal; }

// ---- which instantiation inside a family -------------------------------------------------------------------------
// The policies a call's light_pixel is instantiated with (light_core.hpp): the one place that turns flags into them.  The kernels of
// kernels.hip know the lookup alone (their MIPS parameter: DerivativeChain or Level0, no flag of the other two set); the general
// family and the host build of the bodies (tests/hostsim/host_light.hpp) go through light_variant_visit.
enum class CubeLookup { Level0, DerivativeChain, Gloss };      // CubeLevel0 / CubeChain / CubeGloss (with parallax: CubeGlossBox)
struct LightVariant {
    CubeLookup lookup;
    bool ambientSH;        // AmbientSH, else AmbientConst
    bool splitSum;         // SpecularSplitSum, else SpecularRef
    bool parallax;         // CubeGlossBox in place of CubeGloss (CRYCHIC_LIGHT_CUBE_PARALLAX)
};
inline LightVariant light_variant(uint32_t flags, uint32_t cubeLevels)
{
    const CubeLookup lookup = (flags & CRYCHIC_LIGHT_CUBE_GLOSS) ? CubeLookup::Gloss : cubeLevels > 1u ? CubeLookup::DerivativeChain : CubeLookup::Level0;
    return LightVariant{ lookup, (flags & CRYCHIC_LIGHT_AMBIENT_SH) != 0, (flags & CRYCHIC_LIGHT_ENV_BRDF) != 0, (flags & CRYCHIC_LIGHT_CUBE_PARALLAX) != 0 };
}
// Byte offset behind the cube map that the kernels of a variant with an environment term take after row1 (one argument, so that
// the table and the coefficient block CRYCHIC_CUBE_SH_BYTES before it cost one address): the table's with the split sum, else the
// coefficient block's.
inline size_t light_variant_tail(const LightVariant& v, uint32_t cubeDim, uint32_t cubeLevels)
{
    return v.splitSum ? env_brdf_offset(cubeDim, cubeLevels) : ambient_sh_offset(cubeDim, cubeLevels);
}
// f(Cube(), Ambient(), Specular()) for the variant's policies (value-initialised tags: take their types), once; false and no call
// for a combination no kernel exists for -- SH with the derivative chain, the split sum or the box projection without the gloss
// lookup (the entries of api.cpp refuse them: ambient_sh_check, env_brdf_check, parallax_check).  Eleven combinations: the seven
// without the box projection, and gloss x {const, SH} x {ref, split sum} with it (CubeGlossBox).  The one switch.
template <class F>
inline bool light_variant_visit_all(const LightVariant& v, F&& f)
{
    auto gloss = [&](auto c) {
        if (v.splitSum) { if (v.ambientSH) f(c, AmbientSH(), SpecularSplitSum()); else f(c, AmbientConst(), SpecularSplitSum()); }
        else { if (v.ambientSH) f(c, AmbientSH(), SpecularRef()); else f(c, AmbientConst(), SpecularRef()); }
    };
    switch (v.lookup) {
    case CubeLookup::Level0:
        if (v.splitSum || v.parallax) return false;
        if (v.ambientSH) f(CubeLevel0(), AmbientSH(), SpecularRef()); else f(CubeLevel0(), AmbientConst(), SpecularRef());
        return true;
    case CubeLookup::DerivativeChain:
        if (v.ambientSH || v.splitSum || v.parallax) return false;
        f(CubeChain(), AmbientConst(), SpecularRef());
        return true;
    case CubeLookup::Gloss:
        if (v.parallax) gloss(CubeGlossBox()); else gloss(CubeGloss());
        return true;
    }
    return false;
}
// The seven combinations without the box projection, for a caller that cannot hand a probe volume over (tests/hostsim/host_light.hpp):
// false and no call for a parallax variant.
template <class F>
inline bool light_variant_visit(const LightVariant& v, F&& f)
{
    return !v.parallax && light_variant_visit_all(v, static_cast<F&&>(f));
}

}  // namespace cry
