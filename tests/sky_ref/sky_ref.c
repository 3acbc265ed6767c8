/* sky_ref.c -- the checker of crychic_render_sky and crychic_sky_sun_colour (TEST INFRASTRUCTURE ONLY): plain C written from the
 * definition in include/crychic_hip.h ("procedural sky"), step by step, with none of the kernel's code.  The tone map's table and
 * polynomial are the oracle's own copy (oracle/or_gamma_pow.inc).  Built with -ffp-contract=off: a b + c is fused only where fmaf
 * is written. */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../oracle/or_gamma_pow.inc"

typedef struct {
    float sunDir[3], altitude, sunIntensity, exposure, sunAngularRadius, groundAlbedo;
    uint32_t viewSteps, sunSteps, reserved[2];
} params_t;

/* counters: what the corpus must reach (tests/sky_lib.py COUNTERS) */
enum { N_GROUND, N_SKY, N_DISC, N_LIT, N_BLOCKED, N_SUNLIT_GROUND, N_DARK_GROUND, N_BLACK, N_COUNTERS };

/* ---- the named primitives ---------------------------------------------------------------------------------------------------- */
static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static float rcp(float b)
{
    if (b != b) return b;
    if (fabsf(b) < 1.17549435e-38f) return copysignf(INFINITY, b);
    if (fabsf(b) > 8.50705917e37f) return copysignf(0.0f, b);          /* 2^126 */
    return 1.0f / b;
}
static float len_from_sq(float x)
{
    const float lo = 7.8886090522101181e-31f, hi = 1.2676506002282294e30f;     /* 2^-100, 2^100 */
    if (x != x || x < lo) x = lo;
    if (x > hi) x = hi;
    return sqrtf(x);
}
static float dot3(const float* u, const float* v) { return fmaf(u[2], v[2], fmaf(u[1], v[1], u[0] * v[0])); }
static float det_exp2(float z)
{
    static const float k[7] = { 0.00015406982856802642f, 0.0013400138122960925f, 0.009618260897696018f, 0.05550328269600868f,
                                0.24022649228572845f, 0.6931471824645996f, 1.0f };
    if (z != z) return z;
    if (z < -125.0f) z = -125.0f;
    if (z > 127.0f) z = 127.0f;
    const float n = nearbyintf(z);      /* ties to even: the default rounding mode */
    const float f = z - n;
    float p = k[0];
    for (int i = 1; i < 7; ++i) p = fmaf(p, f, k[i]);
    return ldexpf(p, (int)n);
}
static float max0(float x) { return x > 0.0f ? x : 0.0f; }
static float pow_inv_gamma(float x)
{
    static const float coef[8] = CRY_GAMMA_POW_COEFFS;
    static const float scale[256] = CRY_GAMMA_POW_SCALE;
    if (!(x > -1.17549435e-38f)) return bits(0x7FC00000u);
    const uint32_t b = fbits(x);
    const float u = bits((b & 0x007FFFFFu) | 0x3F800000u) - 1.0f;
    float p = coef[7];
    for (int i = 6; i >= 0; --i) p = fmaf(p, u, coef[i]);
    return scale[(b >> 23) & 255u] * p;
}
static uint32_t unorm8(float x)
{
    float s = (x != x) ? 0.0f : x;
    s = s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
    return (uint32_t)fmaf(s, 255.0f, 0.5f);
}

/* ---- the atmosphere ---------------------------------------------------------------------------------------------------------- */
#define RG 6360.0f
#define RG2 40449600.0f
#define INV_RG 0.000157232702f
#define NHR -0.180336878f
#define NHM -1.20224583f
static const float BETA_R[3] = { 5.8e-3f, 13.5e-3f, 33.1e-3f };
#define BETA_M 21e-3f
static const float TAU_R[3] = { 0.00836763065f, 0.0194763839f, 0.0477532074f };
#define TAU_M 0.0333262533f
#define PHASE_R 0.0596831031f
#define PHASE_M 0.0195609424f
#define INV_PI 0.318309873f

typedef struct {
    float S[3], r0, a0, cT, r0Sy, invNv, invNv2, invNs, invNs2, cosDisc, groundK, sunIntensity, exposure;
    uint32_t Nv, Ns;
} consts_t;

static consts_t host_constants(const params_t* p)
{
    consts_t k;
    const double x = p->sunDir[0], y = p->sunDir[1], z = p->sunDir[2];
    const double len = sqrt(x * x + y * y + z * z);
    k.S[0] = (float)(x / len);
    k.S[1] = (float)(y / len);
    k.S[2] = (float)(z / len);
    const double alt = p->altitude;
    k.r0 = 6360.0f + p->altitude;
    k.a0 = (float)(alt * (12720.0 + alt));
    k.cT = (float)((60.0 - alt) * (12780.0 + alt));
    k.r0Sy = k.r0 * k.S[1];
    k.Nv = p->viewSteps;
    k.Ns = p->sunSteps;
    k.invNv = 1.0f / (float)k.Nv;
    k.invNv2 = k.invNv * k.invNv;
    k.invNs = 1.0f / (float)k.Ns;
    k.invNs2 = k.invNs * k.invNs;
    const double a2 = (double)p->sunAngularRadius * (double)p->sunAngularRadius;
    k.cosDisc = (float)(1.0 - a2 * (0.5 - a2 / 24.0));
    k.groundK = (p->groundAlbedo * INV_PI) * p->sunIntensity;
    k.sunIntensity = p->sunIntensity;
    k.exposure = p->exposure;
    return k;
}

static float height(float q) { return q * rcp(len_from_sq(q + RG2) + RG); }
static int blocked(float q, float bs) { return bs < 0.0f && fmaf(bs, bs, -q) >= 0.0f; }
static float to_shell(float c, float b)
{
    const float sq = len_from_sq(fmaf(b, b, c));
    return b >= 0.0f ? c * rcp(sq + b) : sq - b;
}
/* sample i of N over a segment of length L */
static void sample(uint32_t i, float invN, float invN2, float L, float* t, float* dt)
{
    const float u = ((float)i + 0.5f) * invN;
    *t = L * (u * u);
    *dt = L * ((float)(2u * i + 1u) * invN2);
}
static void sun_depth(const consts_t* k, float q, float bs, float c, float* dR, float* dM)
{
    const float L = to_shell(c, bs);
    const float twob = bs + bs;
    *dR = 0.0f;
    *dM = 0.0f;
    for (uint32_t j = 0; j < k->Ns; ++j) {
        float s, ds;
        sample(j, k->invNs, k->invNs2, L, &s, &ds);
        const float h = height(fmaf(s, s + twob, q));
        *dR = fmaf(det_exp2(h * NHR), ds, *dR);
        *dM = fmaf(det_exp2(h * NHM), ds, *dM);
    }
}
static float trans(int c, float dR, float dM) { return det_exp2(-fmaf(TAU_R[c], dR, TAU_M * dM)); }

static void texel_direction(uint32_t f, uint32_t x, uint32_t y, float rd, float* d)
{
    const float s = (float)(2u * x + 1u) * rd - 1.0f, t = (float)(2u * y + 1u) * rd - 1.0f;
    /* +X (1, -t, -s), -X (-1, -t, s), +Y (s, 1, t), -Y (s, -1, -t), +Z (s, -t, 1), -Z (-s, -t, -1) */
    const float tab[6][3] = { { 1.0f, -t, -s }, { -1.0f, -t, s }, { s, 1.0f, t }, { s, -1.0f, -t }, { s, -t, 1.0f }, { -s, -t, -1.0f } };
    d[0] = tab[f][0];
    d[1] = tab[f][1];
    d[2] = tab[f][2];
}

static uint32_t texel(const consts_t* k, uint32_t f, uint32_t x, uint32_t y, float rd, uint64_t* n)
{
    /* 1 */
    float d[3], v[3];
    texel_direction(f, x, y, rd, d);
    const float inv = rcp(len_from_sq(dot3(d, d)));
    for (int c = 0; c < 3; ++c) v[c] = d[c] * inv;
    const float mu = dot3(v, k->S);
    /* 2 */
    const float b = k->r0 * v[1], twob = b + b;
    const float dg = fmaf(b, b, -k->a0);
    const int ground = b < 0.0f && dg >= 0.0f;
    const float tEnd = ground ? k->a0 * rcp(len_from_sq(dg) - b) : to_shell(k->cT, b);
    n[ground ? N_GROUND : N_SKY]++;
    /* 3 */
    float vR = 0.0f, vM = 0.0f, sR[3] = { 0, 0, 0 }, sM[3] = { 0, 0, 0 };
    for (uint32_t i = 0; i < k->Nv; ++i) {
        float t, dt;
        sample(i, k->invNv, k->invNv2, tEnd, &t, &dt);
        const float w = t * (t + twob);
        const float q = k->a0 + w;
        const float h = height(q);
        const float rhoR = det_exp2(h * NHR) * dt, rhoM = det_exp2(h * NHM) * dt;
        const float mR = fmaf(0.5f, rhoR, vR), mM = fmaf(0.5f, rhoM, vM);
        vR = vR + rhoR;
        vM = vM + rhoM;
        const float bs = fmaf(t, mu, k->r0Sy);
        if (blocked(q, bs)) { n[N_BLOCKED]++; continue; }
        n[N_LIT]++;
        float dR, dM;
        sun_depth(k, q, bs, max0(k->cT - w), &dR, &dM);
        for (int c = 0; c < 3; ++c) {
            const float T = trans(c, mR + dR, mM + dM);
            sR[c] = fmaf(T, rhoR, sR[c]);
            sM[c] = fmaf(T, rhoM, sM[c]);
        }
    }
    /* 4 */
    const float m1 = fmaf(mu, mu, 1.0f);
    const float phR = PHASE_R * m1;
    const float xg = fmaf(-1.52f, mu, 1.5776f);
    const float phM = (PHASE_M * m1) * rcp(xg * len_from_sq(xg));
    float L[3];
    for (int c = 0; c < 3; ++c) L[c] = k->sunIntensity * fmaf(phR * BETA_R[c], sR[c], (phM * BETA_M) * sM[c]);
    /* 5 */
    const int disc = !ground && mu >= k->cosDisc;
    if (disc) n[N_DISC]++;
    if (ground || disc) {
        const float w = tEnd * (tEnd + twob);
        const float q = max0(k->a0 + w);
        const float bs = fmaf(tEnd, mu, k->r0Sy);
        float Tv[3];
        for (int c = 0; c < 3; ++c) Tv[c] = trans(c, vR, vM);
        if (ground && bs > 0.0f) {
            float dR, dM;
            n[N_SUNLIT_GROUND]++;
            sun_depth(k, q, bs, max0(k->cT - w), &dR, &dM);
            for (int c = 0; c < 3; ++c) L[c] = L[c] + ((k->groundK * (bs * INV_RG)) * trans(c, dR, dM)) * Tv[c];
        } else if (ground)
            n[N_DARK_GROUND]++;
        if (disc)
            for (int c = 0; c < 3; ++c) L[c] = fmaf(k->sunIntensity, Tv[c], L[c]);
    }
    /* 6 */
    uint32_t o = 255u << 24;
    for (int c = 0; c < 3; ++c) {
        const float e = L[c] * k->exposure;
        o |= unorm8(pow_inv_gamma(e * rcp(e + 1.0f))) << (8 * c);
    }
    if (o == 255u << 24) n[N_BLACK]++;
    return o;
}

/* Level 0 of faces [face0, face0 + faces) of the dim-texel cube map `cube` (the whole cube's address); counters may be NULL. */
void sky_ref(uint32_t* cube, uint32_t dim, uint32_t face0, uint32_t faces, const params_t* p, uint64_t* counters)
{
    uint64_t scratch[N_COUNTERS];
    uint64_t* n = counters ? counters : scratch;
    const consts_t k = host_constants(p);
    const float rd = rcp((float)dim);
    for (uint32_t f = face0; f < face0 + faces; ++f)
        for (uint32_t y = 0; y < dim; ++y)
            for (uint32_t x = 0; x < dim; ++x) cube[((size_t)f * dim + y) * dim + x] = texel(&k, f, x, y, rd, n);
}

void sky_ref_sun_colour(const params_t* p, float* rgb)
{
    const consts_t k = host_constants(p);
    if (blocked(k.a0, k.r0Sy)) { rgb[0] = rgb[1] = rgb[2] = 0.0f; return; }
    float dR, dM;
    sun_depth(&k, k.a0, k.r0Sy, k.cT, &dR, &dM);
    for (int c = 0; c < 3; ++c) rgb[c] = k.sunIntensity * trans(c, dR, dM);
}
