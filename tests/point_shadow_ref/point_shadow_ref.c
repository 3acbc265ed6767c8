/*
 * point_shadow_ref.c -- TEST INFRASTRUCTURE: the checker of the shadowed point lights (include/crychic_hip.h
 * crychic_deferred_light_point_shadows).  tests/local_light_ref/local_light_ref.c is included unchanged, and with it the frozen
 * oracle's or_light.c: spot_shadow_factor, pbr_spot_light and the oracle's BRDF, sampler, cube and sky helpers are the ones used
 * here.  Added: the cube face step, the shadowed point term and the frame loop; local_light_ref.c's spot_light_pixel is restated
 * with the point loop shadowed.  Built with the oracle's flags (tests/point_shadow_lib.py).
 */
#include "../local_light_ref/local_light_ref.c"

#define PS_MAX_POINT_SHADOWS 4

typedef struct ps_shadows {
    uint32_t count, dim;
    const uint32_t* maps[PS_MAX_POINT_SHADOWS];     /* six dim x dim faces back to back: +X, -X, +Y, -Y, +Z, -Z */
    float M[PS_MAX_POINT_SHADOWS][16];              /* shadowProj[k] transposed (the layout spot_shadow_factor reads) */
} ps_shadows;

/* The face of v = pos - Position (x before y before z on ties; positive when the component is >= 0) and its view coordinates
 * (a, b, c) by the table of crychic_hip.h: +X (-v.z, v.y, v.x), -X (v.z, v.y, -v.x), +Y (v.x, -v.z, v.y), -Y (v.x, v.z, -v.y),
 * +Z (v.x, v.y, v.z), -Z (-v.x, v.y, -v.z). */
static int point_face(const float v[3], float abc[3])
{
    float ax = fabsf(v[0]), ay = fabsf(v[1]), az = fabsf(v[2]);
    int axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    int neg = !(v[axis] >= 0.0f);
    switch (2 * axis + neg) {
    case 0: abc[0] = -v[2]; abc[1] = v[1]; abc[2] = v[0]; break;
    case 1: abc[0] = v[2]; abc[1] = v[1]; abc[2] = -v[0]; break;
    case 2: abc[0] = v[0]; abc[1] = -v[2]; abc[2] = v[1]; break;
    case 3: abc[0] = v[0]; abc[1] = v[2]; abc[2] = -v[1]; break;
    case 4: abc[0] = v[0]; abc[1] = v[1]; abc[2] = v[2]; break;
    default: abc[0] = -v[0]; abc[1] = v[1]; abc[2] = -v[2]; break;
    }
    return 2 * axis + neg;
}
int ps_point_face(const float v[3], float abc[3]) { return point_face(v, abc); }

/* The cube shadow of a point light at `lightPos`: the spot lights' 9-tap factor on face f of the six, at (a, b, c). */
static float point_shadow_factor(const uint32_t* faces, uint32_t dim, const float M[16], const float lightPos[3], const float pos[3])
{
    float v[3] = { pos[0] - lightPos[0], pos[1] - lightPos[1], pos[2] - lightPos[2] }, abc[3];
    int f = point_face(v, abc);
    return spot_shadow_factor(faces + (size_t)f * dim * dim, dim, M, abc);
}
static void transpose16(const float* m, float t[16])
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) t[4 * i + j] = m[4 * j + i];
}
/* shadowProj: 16 floats as crychic_update_point_shadow_transforms writes them (untransposed) */
float ps_point_shadow_factor(const uint32_t* faces, uint32_t dim, const float shadowProj[16], const float lightPos[3], const float pos[3])
{
    float M[16];
    transpose16(shadowProj, M);
    return point_shadow_factor(faces, dim, M, lightPos, pos);
}

/* or_light.c's pbr_point_light with the shadow factor of point light idx < ps->count (evaluated only in range) scaling the term,
 * fma(s * brdf, lightStrength, result); the others keep 1. */
static void pbr_point_light_shadowed(const or_light* L, const float pos[3], const float albedo[3], float roughness, float metalness,
                                     const float normal[3], const float view[3], int flags, const ps_shadows* ps, uint32_t idx,
                                     float result[3])
{
    float l[3] = { L->Position[0] - pos[0], L->Position[1] - pos[1], L->Position[2] - pos[2] };
    float d = or_len(or_dot3(l, l));
    if (d > L->FalloffEnd) return;
    float s = (ps && idx < ps->count) ? point_shadow_factor(ps->maps[idx], ps->dim, ps->M[idx], L->Position, pos) : 1.0f;
    float rd = or_rcp(d);
    float ln[3] = { l[0] * rd, l[1] * rd, l[2] * rd };
    float att = or_saturate(or_div(L->FalloffEnd - d, L->FalloffEnd - L->FalloffStart));
    float vl[3] = { view[0] + ln[0], view[1] + ln[1], view[2] + ln[2] }, halfVec[3];
    or_normalize3(vl, halfVec);
    float hDotv = or_max0(or_dot3(halfVec, view), 0.001f);
    float nDotl = or_max0(or_dot3(normal, ln), 0.001f);
    float nDotv = or_max0(or_dot3(normal, view), 0.001f);
    float nDotvQ = hDotv;
    float D = ndf_ggx(normal, halfVec, roughness);
    float fr = pow5(or_saturate(1.0f - nDotvQ));
    float k = 0.125f * (roughness + 1.0f) * (roughness + 1.0f);
    float G = geometry_schlick_ggx(nDotv, k) * geometry_schlick_ggx(nDotl, k);
    float rdenom = or_rcp(nDotl * ((flags & OR_FIX_Q3) ? nDotv : nDotvQ));
    for (int c = 0; c < 3; ++c) {
        float f0 = or_lerp(0.04f, albedo[c], metalness);
        float F = fmaf(1.0f - f0, fr, f0);
        float fs = 0.25f * D * G * F;
        fs = fs * rdenom;
        float fd = albedo[c] * (1.0f / OR_PI);
        float kd = (1.0f - F) * (1.0f - metalness);
        float brdf = (flags & OR_FIX_Q4) ? kd * fd + fs : fmaf(F, fs, kd * fd);
        float lightStrength = L->Strength[c] * nDotl;
        lightStrength = lightStrength * att;
        result[c] = fmaf(s * brdf, lightStrength, result[c]);
    }
}

/* local_light_ref.c spot_light_pixel, restated with the point loop shadowed (the one duplication the frozen files force). */
static void point_shadow_pixel(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
                               const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                               const uint8_t* cube, uint32_t cubeDim, uint32_t W, uint32_t H, size_t idx,
                               int numDirLights, float pcfRadius, const or_light* pointLights, uint32_t numPointLights,
                               const or_light* spotLights, uint32_t numSpotLights, const ss_shadows* sh, const ps_shadows* ps, int flags,
                               const uint32_t* depth, float lit[4])
{
    const float* G0 = g0 + idx * 4; const float* G1 = g1 + idx * 4; const float* G2 = g2 + idx * 4;
    float posW[3] = { G0[0], G0[1], G0[2] };
    float metalness = G0[3];
    float albedo[3] = { G1[0], G1[1], G1[2] };
    float roughness = G1[3];
    float nraw[3] = { G2[0], G2[1], G2[2] }, normalW[3];
    or_normalize3(nraw, normalW);

    float toEye[3] = { cb->EyePosW[0] - posW[0], cb->EyePosW[1] - posW[1], cb->EyePosW[2] - posW[2] };
    float view[3];
    or_normalize3(toEye, view);
    float fresnelR0[3];
    for (int c = 0; c < 3; ++c) fresnelR0[c] = or_lerp(0.04f, albedo[c], metalness);

    float pos4[4] = { posW[0], posW[1], posW[2], 1.0f };
    float ambientAccess = 1.0f;
    if (ambient) {
        float sp[4];
        or_mul_v4_m(pos4, cb->ViewProjTex, sp);
        float rw = or_rcp(sp[3]);
        ambientAccess = or_ambient_linear_clamp(ambient, W / 2, H / 2, sp[0] * rw, sp[1] * rw);
    }
    float amb[3];
    for (int c = 0; c < 3; ++c) amb[c] = ambientAccess * cb->AmbientLight[c] * albedo[c];

    float shadowFactors[OR_MAX_LIGHTS];
    for (int i = 0; i < OR_MAX_LIGHTS; ++i) shadowFactors[i] = 1.0f;
    static const float radius[4] = { 30.0f, 50.0f, 80.0f, 100.0f };
    float distance = or_len(or_dot3(toEye, toEye));
    for (int j = 0; j < 4; ++j) {
        int blendTerm = (distance - radius[j] < 5.0f) ? 1 : 0;          /* Q1 */
        if (flags & OR_FIX_Q1) blendTerm = fabsf(distance - radius[j]) < 5.0f;
        if (j < 3 && distance < radius[j] && blendTerm != 0) {
            float sp0[4], sp1[4];
            or_mul_v4_m(pos4, cb->ShadowTransforms[j], sp0);
            or_mul_v4_m(pos4, cb->ShadowTransforms[j + 1], sp1);
            float a = pcf_poisson(shadow[j], shadowDim, sp0, pcfRadius);
            float b = pcf_poisson(shadow[j + 1], shadowDim, sp1, pcfRadius);
            shadowFactors[0] = 0.5f * (a + b);
            break;
        } else if (distance < radius[j]) {
            float sp0[4];
            or_mul_v4_m(pos4, cb->ShadowTransforms[j], sp0);
            shadowFactors[0] = pcf_poisson(shadow[j], shadowDim, sp0, pcfRadius);
            break;
        }
    }

    const float shininess = (1.0f - roughness) * 1.0f;
    float direct[3] = { 0.0f, 0.0f, 0.0f };
    for (int i = 0; i < numDirLights; ++i)
        pbr_dir_light(&cb->Lights[i], albedo, roughness, metalness, normalW, view, shadowFactors[i], flags, direct);
    for (uint32_t i = 0; i < numPointLights; ++i)                     /* the point lights, the first ps->count shadowed */
        pbr_point_light_shadowed(&pointLights[i], posW, albedo, roughness, metalness, normalW, view, flags, ps, i, direct);
    for (uint32_t i = 0; i < numSpotLights; ++i)                      /* the extension: spot lights last, in index order */
        pbr_spot_light(&spotLights[i], posW, albedo, roughness, metalness, normalW, view, flags, sh, i, direct);
    for (int c = 0; c < 3; ++c) {
        float d = or_div(direct[c], direct[c] + 1.0f);
        d = or_pow_inv_gamma(d);
        lit[c] = d + amb[c];
    }

    float negv[3] = { -view[0], -view[1], -view[2] }, r[3];
    or_reflect3(negv, normalW, r);
    float refl[4];
    if (OR_CUBE_LEVELS(flags) > 1u) {
        uint32_t x = (uint32_t)(idx % W), y = (uint32_t)(idx / W);
        float lod = reflection_lod(cb, g0, g2, depth, cubeDim, OR_CUBE_LEVELS(flags), W, H, x, y, r);
        or_cube_trilinear(cube, cubeDim, OR_CUBE_LEVELS(flags), r, lod, refl, 4);
    } else
        cube4(cube, cubeDim, r, refl);
    float cosI = or_saturate(or_dot3(normalW, r));
    float f0 = 1.0f - cosI;
    float f5 = f0 * f0 * f0 * f0 * f0;
    for (int c = 0; c < 3; ++c) {
        float fresnel = fmaf(1.0f - fresnelR0[c], f5, fresnelR0[c]);
        lit[c] = fmaf(shininess * fresnel, refl[c], lit[c]);
    }
    lit[3] = 1.0f;
}

/* ss_deferred_light_spots_shadowed plus the first pointShadowCount point lights shadowed by the six faces at pointMaps[k] through
 * shadowProj[k] (16 floats each, untransposed).  pointShadowCount 0 = ss_deferred_light_spots_shadowed. */
void ps_deferred_light_point_shadows(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
                                     const uint32_t* depth, const uint16_t* ambient, const uint32_t* const shadow[4],
                                     uint32_t shadowDim, const uint8_t* cube, uint32_t cubeDim, uint8_t* out_rgba8,
                                     float* radiance_out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                                     int numDirLights, float pcfSearchRadius, int sky, const or_light* pointLights, uint32_t numPointLights,
                                     const or_light* spotLights, uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim,
                                     const uint32_t* const* shadowMaps, uint32_t pointShadowCount, uint32_t pointShadowDim,
                                     const uint32_t* const* pointMaps, const float* shadowProj)
{
    ss_shadows sh;
    memset(&sh, 0, sizeof sh);
    sh.count = shadowCount; sh.dim = shadowMapDim;
    for (uint32_t k = 0; k < shadowCount && k < SS_MAX_SPOT_SHADOWS; ++k) { sh.maps[k] = shadowMaps[k]; sh.T[k] = cb->ShadowTransforms[4 + k]; }
    ps_shadows ps;
    memset(&ps, 0, sizeof ps);
    ps.count = pointShadowCount; ps.dim = pointShadowDim;
    for (uint32_t k = 0; k < pointShadowCount && k < PS_MAX_POINT_SHADOWS; ++k) { ps.maps[k] = pointMaps[k]; transpose16(shadowProj + 16 * k, ps.M[k]); }
    uint32_t row1 = row0 + rows; if (row1 > H) row1 = H;
    static const float clearColor[4] = { 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = (int)row0; y < (int)row1; ++y) {
        for (uint32_t x = 0; x < W; ++x) {
            size_t idx = (size_t)y * W + x;
            float lit[4];
            if ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu)
                point_shadow_pixel(cb, g0, g1, g2, ambient, shadow, shadowDim, cube, cubeDim, W, H, idx, numDirLights, pcfSearchRadius,
                                   pointLights, numPointLights, spotLights, numSpotLights, &sh, &ps, sky, depth, lit);
            else if (sky & 1)
                sky_pixel(cb, cube, cubeDim, OR_CUBE_LEVELS(sky), W, H, x, (uint32_t)y, lit);
            else
                for (int c = 0; c < 4; ++c) lit[c] = clearColor[c];
            if (radiance_out) for (int c = 0; c < 4; ++c) radiance_out[idx * 4 + c] = lit[c];
            for (int c = 0; c < 4; ++c) out_rgba8[idx * 4 + c] = or_to_unorm8(lit[c]);
        }
    }
}
