/*
 * gloss_ref.c -- TEST INFRASTRUCTURE: the checker of the roughness-prefiltered cube map chain and of the glossy reflection lookup
 * (include/crychic_hip.h crychic_cube_prefilter_samples, crychic_prefilter_cube_chain, CRYCHIC_LIGHT_CUBE_GLOSS).
 * tests/point_shadow_ref/point_shadow_ref.c is included unchanged, and through it local_light_ref.c and the frozen oracle's
 * or_light.c: the samplers (or_cube_trilinear), the BRDF, the shadow factors and the sky are the ones used here.  Added: a sample
 * table of its own in double precision, the prefilter, point_shadow_ref.c's pixel restated with the gloss lookup, and the frame
 * loop.  Built with the oracle's flags (tests/gloss_lib.py).
 */
#include "../point_shadow_ref/point_shadow_ref.c"

#define GL_SAMPLES 32

typedef struct gl_table {
    float s[GL_SAMPLES][4];     /* lx, ly, lz (= the weight), lod */
    uint32_t count;
    float rcpW;
} gl_table;

/* van der Corput: the bits of i mirrored behind the binary point */
static double gl_radical_inverse(uint32_t i)
{
    double r = 0.0, f = 0.5;
    for (; i; i >>= 1, f *= 0.5)
        if (i & 1u) r += f;
    return r;
}

/* The table of level k of `levels` for dim-texel faces, from the definition: all in double, stored as float. */
static void gl_build_table(uint32_t dim, uint32_t levels, uint32_t k, gl_table* t)
{
    const double pi = 3.14159265358979323846;
    const double rho = (double)k / (double)(levels - 1u), a2 = rho * rho;
    const double omegaP = 4.0 * pi / (6.0 * (double)dim * (double)dim);
    const double top = (double)(levels - 1u);
    double sum = 0.0;
    memset(t, 0, sizeof *t);
    for (uint32_t i = 0; i < GL_SAMPLES; ++i) {
        const double xi1 = ((double)i + 0.5) / 32.0, xi2 = gl_radical_inverse(i);
        const double cos2 = (1.0 - xi1) / (1.0 + (a2 - 1.0) * xi1), phi = 2.0 * pi * xi2;
        const double w = 2.0 * cos2 - 1.0;
        if (!(w > 0.0)) continue;
        const double cosT = sqrt(cos2), sinT = sqrt(1.0 - cos2);
        const double q = (a2 - 1.0) * cos2 + 1.0;
        const double D = a2 / (pi * q * q);
        const double omegaS = 1.0 / (32.0 * D / 4.0);
        double lod = 0.5 * log2(omegaS / omegaP) + 1.0;
        lod = lod < 0.0 ? 0.0 : (lod > top ? top : lod);
        float* e = t->s[t->count++];
        e[0] = (float)(2.0 * cosT * sinT * cos(phi));
        e[1] = (float)(2.0 * cosT * sinT * sin(phi));
        e[2] = (float)w;
        e[3] = (float)lod;
        sum += w;
    }
    t->rcpW = (float)(1.0 / sum);
}
int gl_prefilter_samples(uint32_t dim, uint32_t levels, uint32_t level, float* samples, uint32_t* count, float* rcpW)
{
    gl_table t;
    if (levels < 2u || level < 1u || level >= levels || dim == 0u) return -1;
    gl_build_table(dim, levels, level, &t);
    memcpy(samples, t.s, sizeof t.s);
    *count = t.count;
    *rcpW = t.rcpW;
    return 0;
}

/* a x b, each component one fma(a, b, -(c d)) */
static void gl_cross(const float a[3], const float b[3], float out[3])
{
    out[0] = fmaf(a[1], b[2], -(a[2] * b[1]));
    out[1] = fmaf(a[2], b[0], -(a[0] * b[2]));
    out[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}
/* The direction of the centre of texel (x, y) of face f of a d x d level: the inverse of or_cube_linear's face table. */
static void gl_texel_direction(uint32_t f, uint32_t x, uint32_t y, uint32_t d, float r[3])
{
    float rd = or_rcp((float)d);
    float s = (float)(2u * x + 1u) * rd - 1.0f, t = (float)(2u * y + 1u) * rd - 1.0f;
    switch (f) {
    case 0: r[0] = 1.0f; r[1] = -t; r[2] = -s; break;       /* +X: sc = -z, tc = -y */
    case 1: r[0] = -1.0f; r[1] = -t; r[2] = s; break;       /* -X: sc = z, tc = -y */
    case 2: r[0] = s; r[1] = 1.0f; r[2] = t; break;         /* +Y: sc = x, tc = z */
    case 3: r[0] = s; r[1] = -1.0f; r[2] = -t; break;       /* -Y: sc = x, tc = -z */
    case 4: r[0] = s; r[1] = -t; r[2] = 1.0f; break;        /* +Z: sc = x, tc = -y */
    default: r[0] = -s; r[1] = -t; r[2] = -1.0f; break;     /* -Z: sc = -x, tc = -y */
    }
}
static void gl_prefilter_texel(const uint8_t* src, uint32_t dim, uint32_t levels, uint32_t d, uint32_t f, uint32_t x, uint32_t y,
                               const gl_table* t, uint8_t out[4])
{
    float dir[3], N[3], T[3], B[3], c[4], acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    gl_texel_direction(f, x, y, d, dir);
    or_normalize3(dir, N);
    const float upZ[3] = { 0.0f, 0.0f, 1.0f }, upX[3] = { 1.0f, 0.0f, 0.0f };
    float uxn[3];
    gl_cross(fabsf(N[2]) < 0.999f ? upZ : upX, N, uxn);
    or_normalize3(uxn, T);
    gl_cross(N, T, B);
    for (uint32_t i = 0; i < t->count; ++i) {
        const float* e = t->s[i];
        float L[3];
        for (int j = 0; j < 3; ++j) L[j] = fmaf(e[2], N[j], fmaf(e[1], B[j], e[0] * T[j]));
        or_cube_trilinear(src, dim, levels, L, e[3], c, 4);
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(e[2], c[j], acc[j]);
    }
    for (int j = 0; j < 4; ++j) out[j] = or_to_unorm8(acc[j] * t->rcpW);
}
/* dst: the prefiltered chain of src (dim, levels); the two do not overlap. */
void gl_prefilter_chain(const uint8_t* src, uint8_t* dst, uint32_t dim, uint32_t levels)
{
    memcpy(dst, src, (size_t)6u * dim * dim * 4u);
    for (uint32_t k = 1; k < levels; ++k) {
        gl_table t;
        gl_build_table(dim, levels, k, &t);
        uint32_t d = or_cube_level_dim(dim, k);
        uint8_t* level = dst + or_cube_level_offset(dim, k);
#pragma omp parallel for schedule(static)
        for (int row = 0; row < (int)(6u * d); ++row)
            for (uint32_t x = 0; x < d; ++x)
                gl_prefilter_texel(src, dim, levels, d, (uint32_t)row / d, x, (uint32_t)row % d, &t, level + ((size_t)row * d + x) * 4u);
    }
}

/* The shadowed local-light pixel of point_shadow_ref.c (with no lights: or_light.c's plain pixel, as the tests of the frozen checkers
 * show), restated with the gloss lookup: DeferredShading.hlsl:95 reads the prefiltered chain at lod = saturate(roughness) * (levels - 1),
 * trilinear; everything else -- shininess and the Fresnel factor of :96-97 included -- is as written there. */
static void gl_gloss_pixel(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
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
    float lod = or_saturate(roughness) * (float)(OR_CUBE_LEVELS(flags) - 1u);      /* NaN -> 0 */
    or_cube_trilinear(cube, cubeDim, OR_CUBE_LEVELS(flags), r, lod, refl, 4);
    float cosI = or_saturate(or_dot3(normalW, r));
    float f0 = 1.0f - cosI;
    float f5 = f0 * f0 * f0 * f0 * f0;
    for (int c = 0; c < 3; ++c) {
        float fresnel = fmaf(1.0f - fresnelR0[c], f5, fresnelR0[c]);
        lit[c] = fmaf(shininess * fresnel, refl[c], lit[c]);
    }
    lit[3] = 1.0f;
}

/* ps_deferred_light_point_shadows with CRYCHIC_LIGHT_CUBE_GLOSS: `sky` (the flags word) carries the flag and
 * CRYCHIC_LIGHT_CUBE_LEVELS(n), n > 1; covered pixels take gl_gloss_pixel, the sky reads level 0 alone. */
void gl_deferred_light_gloss(const or_pass_constants* cb, const float* g0, const float* g1, const float* g2,
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
                gl_gloss_pixel(cb, g0, g1, g2, ambient, shadow, shadowDim, cube, cubeDim, W, H, idx, numDirLights, pcfSearchRadius,
                                   pointLights, numPointLights, spotLights, numSpotLights, &sh, &ps, sky, depth, lit);
            else if (sky & 1)
                sky_pixel(cb, cube, cubeDim, 1u, W, H, x, (uint32_t)y, lit);
            else
                for (int c = 0; c < 4; ++c) lit[c] = clearColor[c];
            if (radiance_out) for (int c = 0; c < 4; ++c) radiance_out[idx * 4 + c] = lit[c];
            for (int c = 0; c < 4; ++c) out_rgba8[idx * 4 + c] = or_to_unorm8(lit[c]);
        }
    }
}
