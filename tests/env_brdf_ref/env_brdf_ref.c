/*
 * env_brdf_ref.c -- TEST INFRASTRUCTURE: the checker of the environment BRDF table and of the lighting pixel whose reflection term is
 * weighed by it (include/crychic_hip.h "environment BRDF table", crychic_build_env_brdf, CRYCHIC_LIGHT_ENV_BRDF).
 * tests/env_sh_ref/env_sh_ref.c is included unchanged, and through it gloss_ref.c, point_shadow_ref.c, local_light_ref.c and the frozen
 * oracle's or_light.c: the samplers, the BRDF of the direct lights, the shadow factors, the sky and the SH ambient term are the ones
 * used here.  Added: the table restated sample by sample in plain loops (one running sum per quantity, no reduction tree) with the
 * definition's bounds asserted, the table's bilinear lookup, es_pixel restated with the split-sum weight and either ambient term, and
 * the frame loop.  Built with the oracle's flags (tests/env_brdf_lib.py).
 */
#include "../env_sh_ref/env_sh_ref.c"

#define EB_FLAG 0x100000
#define EB_AMBIENT_SH 0x8000
#define EB_TABLE_BYTES 4096u

static const uint32_t eb_cos_bits[8] = { 0x3f7ec46du, 0x3f74fa0bu, 0x3f61c598u, 0x3f45e403u, 0x3f226799u, 0x3ef15aeau, 0x3e94a031u, 0x3dc8bd36u };

static float eb_cos(uint32_t t)
{
    uint32_t u = t < 8u ? eb_cos_bits[t] : (eb_cos_bits[15u - t] ^ 0x80000000u);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

/* The two integer sums of texel (row j, column i) over the samples with index in [first, last) of the 4096 (index = 16 s + t), in
 * units of 2^-24.  The whole texel is [0, 4096); a test adds the sums of parts to show that the grouping does not matter.  Returns the
 * largest term met (the definition's bound: below 19.5; asserted below 64), or -1 if a term was negative or not finite. */
float eb_sums(uint32_t j, uint32_t i, uint32_t first, uint32_t last, int64_t sums[2])
{
    float rho = ((float)j + 0.5f) / 32.0f, mu = ((float)i + 0.5f) / 32.0f;
    float a2m1 = fmaf(rho, rho, -1.0f);
    float k = 0.125f * (rho + 1.0f) * (rho + 1.0f);
    float omk = 1.0f - k;
    float vz = mu;
    float vx = or_len(fmaf(-mu, mu, 1.0f));
    float gV = or_rcp(fmaf(vz, omk, k));
    float worst = 0.0f;
    sums[0] = 0; sums[1] = 0;
    for (uint32_t n = first; n < last; ++n) {
        uint32_t s = n / 16u, t = n % 16u;
        float xi = ((float)s + 0.5f) / 256.0f;
        float c2 = (1.0f - xi) * or_rcp(fmaf(a2m1, xi, 1.0f));
        float c = or_len(c2);
        float sn = or_len(1.0f - c2);
        float rc = or_rcp(c);
        float voh = fmaf(vx, sn * eb_cos(t), vz * c);
        float lz = fmaf(2.0f * voh, c, -vz);
        if (!(lz > 0.0f)) continue;
        float gL = lz * or_rcp(fmaf(lz, omk, k));
        float gv = ((gV * gL) * voh) * rc;
        float f = 1.0f - or_saturate(voh);
        float fc = f * f;
        fc = fc * f;
        fc = fc * f;
        fc = fc * f;
        float tB = fc * gv;
        float tA = (1.0f - fc) * gv;
        if (!(tA >= 0.0f && tB >= 0.0f && tA < 64.0f && tB < 64.0f)) return -1.0f;
        if (tA > worst) worst = tA;
        if (tB > worst) worst = tB;
        sums[0] += (int64_t)rintf(tA * 16777216.0f);
        sums[1] += (int64_t)rintf(tB * 16777216.0f);
    }
    return worst;
}

/* the dword of finished sums */
uint32_t eb_pack(const int64_t sums[2])
{
    float A = (float)((double)sums[0] / 68719476736.0), B = (float)((double)sums[1] / 68719476736.0);      /* 2^36 */
    return (uint32_t)or_to_unorm16(A) | ((uint32_t)or_to_unorm16(B) << 16);
}

/* The 1024 dwords and (if sums is not NULL) the 2048 sums, [texel][A, B].  Returns 0, or -1 when a bound the definition states does
 * not hold: a term outside [0, 64), A + B > 1 or B > 0.15. */
int eb_table(uint32_t table[1024], int64_t* sums)
{
    for (uint32_t j = 0; j < 32u; ++j)
        for (uint32_t i = 0; i < 32u; ++i) {
            int64_t s[2];
            if (eb_sums(j, i, 0u, 4096u, s) < 0.0f) return -1;
            uint32_t w = eb_pack(s);
            if ((w & 0xFFFFu) + (w >> 16) > 65535u) return -1;              /* A + B <= 1 */
            if ((w >> 16) > 9830u) return -1;                              /* B <= 0.15 */
            table[j * 32u + i] = w;
            if (sums) { sums[2u * (j * 32u + i)] = s[0]; sums[2u * (j * 32u + i) + 1u] = s[1]; }
        }
    return 0;
}

/* (A, B) of a table at (u, v) = (saturate(N.V), saturate(roughness)): bilinear, indices clamped to the table. */
void eb_lookup(const uint32_t* table, float nDotV, float roughness, float ab[2])
{
    float u = or_saturate(nDotV), v = or_saturate(roughness);
    float tx = fmaf(u, 32.0f, -0.5f), ty = fmaf(v, 32.0f, -0.5f);
    float flx = floorf(tx), fly = floorf(ty);
    float fx = tx - flx, fy = ty - fly;
    int x0 = or_clampi((int)flx, 0, 31), x1 = or_clampi((int)flx + 1, 0, 31);
    int y0 = or_clampi((int)fly, 0, 31), y1 = or_clampi((int)fly + 1, 0, 31);
    uint32_t t00 = table[y0 * 32 + x0], t10 = table[y0 * 32 + x1], t01 = table[y1 * 32 + x0], t11 = table[y1 * 32 + x1];
    ab[0] = or_bilerp(or_unorm16((uint16_t)(t00 & 0xFFFFu)), or_unorm16((uint16_t)(t10 & 0xFFFFu)), or_unorm16((uint16_t)(t01 & 0xFFFFu)),
                      or_unorm16((uint16_t)(t11 & 0xFFFFu)), fx, fy);
    ab[1] = or_bilerp(or_unorm16((uint16_t)(t00 >> 16)), or_unorm16((uint16_t)(t10 >> 16)), or_unorm16((uint16_t)(t01 >> 16)),
                      or_unorm16((uint16_t)(t11 >> 16)), fx, fy);
}

/* where the table follows a cube map of `levels` levels */
size_t eb_table_offset(uint32_t dim, uint32_t levels) { return es_tail_offset(dim, levels) + ES_TAIL_BYTES; }

/* es_pixel restated with the reflection weighed by the table: lit_c = fma(fma(R0_c, A, B), refl_c, tm_c); shininess and the Fresnel
 * term of the mirror direction do not appear.  The ambient colour is AmbientLight's (coeffs == NULL) or the SH block's.  The lookup
 * is the gloss lookup. */
static void eb_pixel(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
                     const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                     const uint8_t* cube, uint32_t cubeDim, const float* coeffs, const uint32_t* table, uint32_t W, uint32_t H,
                     size_t idx, int numDirLights, float pcfRadius, const or_light* pointLights, uint32_t numPointLights,
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
    float lod = or_saturate(roughness) * (float)(OR_CUBE_LEVELS(flags) - 1u);      /* NaN -> 0 */
    or_cube_trilinear(cube, cubeDim, OR_CUBE_LEVELS(flags), r, lod, refl, 4);
    float ab[2];
    eb_lookup(table, or_dot3(normalW, view), roughness, ab);
    for (int c = 0; c < 3; ++c) {
        float spec = fmaf(fresnelR0[c], ab[0], ab[1]);
        lit[c] = fmaf(spec, refl[c], lit[c]);
    }
    lit[3] = 1.0f;
}

/* R0 of a pixel as the pass computes it (a test asserts its known answers) */
void eb_r0(const float albedo[3], float metalness, float r0[3])
{
    for (int c = 0; c < 3; ++c) r0[c] = or_lerp(0.04f, albedo[c], metalness);
}

/* es_deferred_light_sh's arguments with CRYCHIC_LIGHT_ENV_BRDF | CRYCHIC_LIGHT_CUBE_GLOSS | CRYCHIC_LIGHT_CUBE_LEVELS(n > 1), with or
 * without CRYCHIC_LIGHT_AMBIENT_SH: `cube` holds the gloss chain, at es_tail_offset the environment tail (read only with the SH
 * flag) and at eb_table_offset the 1024 dwords of the table. */
void eb_deferred_light_spec(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
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
    uint32_t mine[1024];
    memcpy(coeffs, cube + es_tail_offset(cubeDim, OR_CUBE_LEVELS(sky)), sizeof coeffs);
    memcpy(mine, cube + eb_table_offset(cubeDim, OR_CUBE_LEVELS(sky)), sizeof mine);
    const float* shc = (sky & EB_AMBIENT_SH) ? coeffs : NULL;
    uint32_t row1 = row0 + rows; if (row1 > H) row1 = H;
    static const float clearColor[4] = { 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = (int)row0; y < (int)row1; ++y) {
        for (uint32_t x = 0; x < W; ++x) {
            size_t idx = (size_t)y * W + x;
            float lit[4];
            if ((depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu)
                eb_pixel(cb, g0, g1, g2, ambient, shadow, shadowDim, cube, cubeDim, shc, mine, W, H, idx, numDirLights, pcfSearchRadius,
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
