/*
 * parallax_ref.c -- TEST INFRASTRUCTURE: the checker of the box-projected environment probe and of the lighting pixel whose
 * reflection lookup is corrected by it (include/crychic_hip.h "probe volume", CRYCHIC_LIGHT_CUBE_PARALLAX).
 * tests/env_brdf_ref/env_brdf_ref.c is included unchanged, and through it env_sh_ref.c, gloss_ref.c, point_shadow_ref.c,
 * local_light_ref.c and the frozen oracle's or_light.c: the samplers, the BRDF of the direct lights, the shadow factors, the sky, the
 * SH ambient term and the table's lookup are the ones used here.  Added: the correction written from the definition, component by
 * component, the gloss pixel restated with it and with either ambient term and either weight of the reflection, and the frame
 * loop.  Built with the oracle's flags (tests/parallax_lib.py).
 */
#include "../env_brdf_ref/env_brdf_ref.c"

#define PX_FLAG 0x200000
#define PX_PROBE_OFFSET 368u
#define PX_PROBE_BYTES 48u

/* where the probe volume sits behind a cube map of `levels` levels */
size_t px_probe_offset(uint32_t dim, uint32_t levels) { return es_tail_offset(dim, levels) + PX_PROBE_OFFSET; }

/* The correction.  probe: the twelve floats of the volume, c, bmin, bmax as float4.  Returns t through *tOut (if not NULL): +inf
 * when nothing is usable. */
void px_correct(const float p[3], const float r[3], const float probe[12], float out[3], float* tOut)
{
    const float* c = probe;
    const float* bmin = probe + 4;
    const float* bmax = probe + 8;
    float t = INFINITY;
    for (int k = 0; k < 3; ++k) {
        if (!(fabsf(r[k]) >= 0x1p-126f)) continue;             /* zero, subnormal or NaN: skipped */
        float e = (r[k] < 0.0f ? bmin[k] : bmax[k]) - p[k];
        float tk = e * or_rcp(r[k]);
        t = (tk < t) ? tk : t;                                  /* a NaN tk loses */
    }
    t = (t > 0.0f) ? t : 0.0f;
    if (tOut) *tOut = t;
    if (!(t < INFINITY)) { out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; return; }
    for (int k = 0; k < 3; ++k) {
        float h = fmaf(r[k], t, p[k]);
        out[k] = h - c[k];
    }
}

/* The gloss pixel (gl_gloss_pixel / es_pixel / eb_pixel) restated with the corrected direction handed to the cube lookup and to
 * nothing else.  coeffs: the SH block or NULL (AmbientLight); table: the split-sum table or NULL (shininess and Fresnel as written). */
static void px_pixel(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
                     const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                     const uint8_t* cube, uint32_t cubeDim, const float* coeffs, const uint32_t* table, const float* probe, uint32_t W,
                     uint32_t H, size_t idx, int numDirLights, float pcfRadius, const or_light* pointLights, uint32_t numPointLights,
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
    float amb[3];
    if (coeffs) {
        float e[3];
        es_irradiance(coeffs, normalW, e);
        for (int c = 0; c < 3; ++c) amb[c] = ambientAccess * e[c] * albedo[c];
    } else {
        for (int c = 0; c < 3; ++c) amb[c] = ambientAccess * cb->AmbientLight[c] * albedo[c];
    }

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

    float negv[3] = { -view[0], -view[1], -view[2] }, r[3], rl[3];
    or_reflect3(negv, normalW, r);
    px_correct(posW, r, probe, rl, NULL);                       /* the lookup's direction; everything below stays on r */
    float refl[4];
    float lod = or_saturate(roughness) * (float)(OR_CUBE_LEVELS(flags) - 1u);      /* NaN -> 0 */
    or_cube_trilinear(cube, cubeDim, OR_CUBE_LEVELS(flags), rl, lod, refl, 4);
    if (table) {
        float ab[2];
        eb_lookup(table, or_dot3(normalW, view), roughness, ab);
        for (int c = 0; c < 3; ++c) {
            float spec = fmaf(fresnelR0[c], ab[0], ab[1]);
            lit[c] = fmaf(spec, refl[c], lit[c]);
        }
    } else {
        float cosI = or_saturate(or_dot3(normalW, r));
        float f0 = 1.0f - cosI;
        float f5 = f0 * f0 * f0 * f0 * f0;
        for (int c = 0; c < 3; ++c) {
            float fresnel = fmaf(1.0f - fresnelR0[c], f5, fresnelR0[c]);
            lit[c] = fmaf(shininess * fresnel, refl[c], lit[c]);
        }
    }
    lit[3] = 1.0f;
}

/* eb_deferred_light_spec's arguments with CRYCHIC_LIGHT_CUBE_PARALLAX | CRYCHIC_LIGHT_CUBE_GLOSS | CRYCHIC_LIGHT_CUBE_LEVELS(n > 1), with
 * or without CRYCHIC_LIGHT_AMBIENT_SH and CRYCHIC_LIGHT_ENV_BRDF: `cube` holds the gloss chain, at es_tail_offset the environment tail
 * (its coefficient block read only with the SH flag, the probe volume at px_probe_offset always) and, with the split-sum flag, at
 * eb_table_offset the 1024 dwords of the table. */
void px_deferred_light_parallax(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
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
    float coeffs[36], probe[12];
    uint32_t mine[1024];
    memcpy(coeffs, cube + es_tail_offset(cubeDim, OR_CUBE_LEVELS(sky)), sizeof coeffs);
    memcpy(probe, cube + px_probe_offset(cubeDim, OR_CUBE_LEVELS(sky)), sizeof probe);
    if (sky & EB_FLAG) memcpy(mine, cube + eb_table_offset(cubeDim, OR_CUBE_LEVELS(sky)), sizeof mine);      /* no table behind the tail otherwise */
    const float* shc = (sky & EB_AMBIENT_SH) ? coeffs : NULL;
    const uint32_t* table = (sky & EB_FLAG) ? mine : NULL;
    uint32_t row1 = row0 + rows; if (row1 > H) row1 = H;
    static const float clearColor[4] = { 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = (int)row0; y < (int)row1; ++y) {
        for (uint32_t x = 0; x < W; ++x) {
            size_t idx = (size_t)y * W + x;
            float lit[4];
            if ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu)
                px_pixel(cb, g0, g1, g2, ambient, shadow, shadowDim, cube, cubeDim, shc, table, probe, W, H, idx, numDirLights,
                         pcfSearchRadius, pointLights, numPointLights, spotLights, numSpotLights, &sh, &ps, sky, lit);
            else if (sky & 1)
                sky_pixel(cb, cube, cubeDim, 1u, W, H, x, (uint32_t)y, lit);
            else
                for (int c = 0; c < 4; ++c) lit[c] = clearColor[c];
            if (radiance_out) for (int c = 0; c < 4; ++c) radiance_out[idx * 4 + c] = lit[c];
            for (int c = 0; c < 4; ++c) out_rgba8[idx * 4 + c] = or_to_unorm8(lit[c]);
        }
    }
}
