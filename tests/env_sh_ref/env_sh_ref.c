/*
 * env_sh_ref.c -- TEST INFRASTRUCTURE: the checker of the SH9 irradiance projection of a cube map level and of the lighting pixel
 * whose ambient colour comes from it (include/crychic_hip.h "SH9 irradiance", crychic_project_cube_sh, CRYCHIC_LIGHT_AMBIENT_SH).
 * tests/gloss_ref/gloss_ref.c is included unchanged, and through it point_shadow_ref.c, local_light_ref.c and the frozen oracle's
 * or_light.c: the samplers, the BRDF, the shadow factors, the sky and the texel directions are the ones used here.  Added: the
 * projection restated texel by texel in plain loops (one running sum per quantity, no reduction tree), gloss_ref.c's pixel restated
 * with the SH ambient term and either lookup, and the frame loop.  Built with the oracle's flags (tests/env_sh_lib.py).
 */
#include "../gloss_ref/gloss_ref.c"

#define ES_TAIL_BYTES 512u

static const double es_K[9] = { 1.0, 2.0, 2.0, 2.0, 15.0 / 4.0, 15.0 / 4.0, 5.0 / 16.0, 15.0 / 4.0, 15.0 / 16.0 };

/* the nine monomials of a unit vector */
static void es_basis(const float n[3], float b[9])
{
    b[0] = 1.0f; b[1] = n[1]; b[2] = n[2]; b[3] = n[0];
    b[4] = n[0] * n[1];
    b[5] = n[1] * n[2];
    b[6] = fmaf(3.0f * n[2], n[2], -1.0f);
    b[7] = n[0] * n[2];
    b[8] = fmaf(n[0], n[0], -(n[1] * n[1]));
}

/* One texel's ten quantised terms: q[0..8] and the weight q[9], in units of 2^-20. */
static void es_texel_terms(uint32_t f, uint32_t x, uint32_t y, uint32_t d, int64_t q[10])
{
    float dir[3], n[3], b[9];
    gl_texel_direction(f, x, y, d, dir);
    float r2 = or_dot3(dir, dir);
    or_normalize3(dir, n);
    float w = or_rcp(r2 * sqrtf(r2));
    es_basis(n, b);
    for (int m = 0; m < 9; ++m) {
        float t = w * b[m];
        q[m] = (int64_t)rintf(t * 1048576.0f);
    }
    q[9] = (int64_t)rintf(w * 1048576.0f);
}

/* The 28 integer sums of the texels with index in [first, last) of the level (face-major, then rows): sums[3 m + c], sums[27] = S_w.
 * The whole level is [0, 6 d^2); a test adds the sums of two parts to show that the order does not matter. */
void es_sums(const uint8_t* level, uint32_t d, uint32_t first, uint32_t last, int64_t sums[28])
{
    for (int k = 0; k < 28; ++k) sums[k] = 0;
    for (uint32_t i = first; i < last; ++i) {
        uint32_t f = i / (d * d), in = i % (d * d);
        int64_t q[10];
        es_texel_terms(f, in % d, in / d, d, q);
        for (int m = 0; m < 9; ++m)
            for (int c = 0; c < 3; ++c) sums[3 * m + c] += q[m] * (int64_t)level[(size_t)i * 4u + c];
        sums[27] += q[9];
    }
}
/* The coefficient block of finished sums: nine float4, the fourth components 0. */
void es_coefficients(const int64_t sums[28], float coeffs[36])
{
    for (int m = 0; m < 9; ++m) {
        for (int c = 0; c < 3; ++c) {
            double num = (double)sums[3 * m + c] * es_K[m];
            double den = (double)sums[27] * 255.0;
            coeffs[4 * m + c] = (float)(num / den);
        }
        coeffs[4 * m + 3] = 0.0f;
    }
}
void es_project(const uint8_t* level, uint32_t d, float coeffs[36])
{
    int64_t sums[28];
    es_sums(level, d, 0u, 6u * d * d, sums);
    es_coefficients(sums, coeffs);
}

/* E(n) of a coefficient block for a unit vector n, per channel, after the clamp. */
void es_irradiance(const float coeffs[36], const float n[3], float e[3])
{
    float b[9];
    es_basis(n, b);
    for (int c = 0; c < 3; ++c) {
        float v = coeffs[c];
        for (int m = 1; m < 9; ++m) v = fmaf(coeffs[4 * m + c], b[m], v);
        e[c] = or_max0(v, 0.0f);            /* NaN -> 0 */
    }
}

/* where the environment tail follows a cube map of `levels` levels (0 counts as 1) */
size_t es_tail_offset(uint32_t dim, uint32_t levels)
{
    size_t n = 0;
    for (uint32_t k = 0; k < (levels ? levels : 1u); ++k) { size_t d = or_cube_level_dim(dim, k); n += 6u * d * d * 4u; }
    return (n + 15u) / 16u * 16u;
}

/* gloss_ref.c's pixel restated with the ambient colour from the coefficient block: amb_c = ambientAccess * E_c(normalW) * albedo_c;
 * AmbientLight is not read.  The reflection lookup is level 0 alone (no chain) or the gloss lookup (OR_CUBE_LEVELS(flags) > 1). */
static void es_pixel(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
                     const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                     const uint8_t* cube, uint32_t cubeDim, const float* coeffs, uint32_t W, uint32_t H, size_t idx,
                     int numDirLights, float pcfRadius, const or_light* pointLights, uint32_t numPointLights,
                     const or_light* spotLights, uint32_t numSpotLights, const ss_shadows* sh, const ps_shadows* ps, int flags,
                     float lit[4])
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
    float e[3], amb[3];
    es_irradiance(coeffs, normalW, e);
    for (int c = 0; c < 3; ++c) amb[c] = ambientAccess * e[c] * albedo[c];

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
    for (uint32_t i = 0; i < numPointLights; ++i)
        pbr_point_light_shadowed(&pointLights[i], posW, albedo, roughness, metalness, normalW, view, flags, ps, i, direct);
    for (uint32_t i = 0; i < numSpotLights; ++i)
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
        float lod = or_saturate(roughness) * (float)(OR_CUBE_LEVELS(flags) - 1u);      /* NaN -> 0 */
        or_cube_trilinear(cube, cubeDim, OR_CUBE_LEVELS(flags), r, lod, refl, 4);
    } else {
        or_cube_linear(cube, cubeDim, r, refl, 4);
    }
    float cosI = or_saturate(or_dot3(normalW, r));
    float f0 = 1.0f - cosI;
    float f5 = f0 * f0 * f0 * f0 * f0;
    for (int c = 0; c < 3; ++c) {
        float fresnel = fmaf(1.0f - fresnelR0[c], f5, fresnelR0[c]);
        lit[c] = fmaf(shininess * fresnel, refl[c], lit[c]);
    }
    lit[3] = 1.0f;
}

/* gl_deferred_light_gloss's arguments with CRYCHIC_LIGHT_AMBIENT_SH: `cube` holds the cube map (with CRYCHIC_LIGHT_CUBE_LEVELS(n > 1)
 * a gloss chain) and, at es_tail_offset(cubeDim, levels), the environment tail whose first 36 floats are the coefficient block. */
void es_deferred_light_sh(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
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
    float coeffs[36];
    memcpy(coeffs, cube + es_tail_offset(cubeDim, OR_CUBE_LEVELS(sky)), sizeof coeffs);
    uint32_t row1 = row0 + rows; if (row1 > H) row1 = H;
    static const float clearColor[4] = { 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = (int)row0; y < (int)row1; ++y) {
        for (uint32_t x = 0; x < W; ++x) {
            size_t idx = (size_t)y * W + x;
            float lit[4];
            if ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu)
                es_pixel(cb, g0, g1, g2, ambient, shadow, shadowDim, cube, cubeDim, coeffs, W, H, idx, numDirLights, pcfSearchRadius,
                         pointLights, numPointLights, spotLights, numSpotLights, &sh, &ps, sky, lit);
            else if (sky & 1)
                sky_pixel(cb, cube, cubeDim, 1u, W, H, x, (uint32_t)y, lit);
            else
                for (int c = 0; c < 4; ++c) lit[c] = clearColor[c];
            if (radiance_out) for (int c = 0; c < 4; ++c) radiance_out[idx * 4 + c] = lit[c];
            for (int c = 0; c < 4; ++c) out_rgba8[idx * 4 + c] = or_to_unorm8(lit[c]);
        }
    }
}
