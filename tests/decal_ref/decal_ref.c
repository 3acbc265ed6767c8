/* decal_ref.c -- the checker of crychic_apply_decals (TEST INFRASTRUCTURE ONLY): plain C written from the definition in
 * include/crychic_hip.h, step by step, with its own restatement of every primitive.  It includes nothing of csrc/ and shares no code
 * with the kernel: every pixel walks every decal, there is no tile and no cull.  Built with -ffp-contract=off: a product and a sum
 * are fused exactly where fmaf is written.
 * It counts the branches of the definition it takes (COUNTERS in tests/decal_lib.py, in this order). */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { N_UNCOVERED, N_OUTSIDE_BOUNDS, N_OUTSIDE_BOX, N_FADE_ZERO, N_FADE_PARTIAL, N_FADE_ONE, N_A_NOT_POSITIVE, N_ONE_LEVEL, N_LOD_LOW, N_LOD_INTERIOR,
       N_LOD_HIGH, N_CLAMP_LEFT, N_CLAMP_RIGHT, N_CLAMP_TOP, N_CLAMP_BOTTOM, N_STORE_ALBEDO, N_STORE_ROUGHNESS, N_STORE_METALNESS, N_STORE_NORMAL,
       N_NORMAL_NO_MAP, N_BAD_TEXTURE, N_NONFINITE_POSITION, N_COUNTERS };

typedef struct {
    float invWorld[12], boundsMin[3], boundsMax[3], tangentW[3], bitangentW[3], normalW[3], tint[3], opacity, roughness, metalness, fadeScale,
          fadeBias, texelsPerUnit;
    uint32_t texture, normalTexture, flags, reserved;
} ref_decal;
typedef struct { const uint8_t* texels; uint32_t width, height, mipLevels; } ref_texture;
typedef char ref_decal_is_160_bytes[sizeof(ref_decal) == 160 ? 1 : -1];

static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

float decal_ref_h2f(uint16_t h)
{
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 0) { const float f = (float)m * 5.9604644775390625e-8f; return s ? -f : f; }
    if (e == 31) return bits(s | 0x7F800000u | (m << 13));
    return bits(s | ((e + 112u) << 23) | (m << 13));
}

uint16_t decal_ref_f2h(float f)
{
    const uint32_t u = fbits(f), s = (u >> 16) & 0x8000u, x = u & 0x7FFFFFFFu;
    int e;
    uint32_t mant, shift, h, rem, half;
    if (x > 0x7F800000u) return (uint16_t)(s | 0x7E00u | ((x >> 13) & 0x3FFu));
    if (x == 0x7F800000u) return (uint16_t)(s | 0x7C00u);
    e = (int)(x >> 23) - 127;
    if (e > 15) return (uint16_t)(s | 0x7C00u);
    if (e < -26) return (uint16_t)s;
    mant = (x & 0x7FFFFFu) | 0x800000u;
    shift = e >= -14 ? 13u : (uint32_t)(13 + (-14 - e));
    h = mant >> shift;
    rem = mant & ((1u << shift) - 1u);
    half = 1u << (shift - 1u);
    if (e >= -14) h = (h & 0x3FFu) | ((uint32_t)(e + 15) << 10);
    if (rem > half || (rem == half && (h & 1u))) ++h;       /* a carry runs into the exponent, up to infinity */
    return (uint16_t)(s | h);
}

static float ref_mulcol1(const float p[3], const float* m) { return fmaf(p[2], m[2], fmaf(p[1], m[1], p[0] * m[0])) + m[3]; }
static float ref_dot3(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
static float ref_lerp(float a, float b, float t) { return fmaf(t, b - a, a); }
static float ref_saturate(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

static void ref_normalize3(const float v[3], float out[3])
{
    float L = ref_dot3(v, v), inv;
    if (L != L) L = 7.8886090522101181e-31f;
    if (L < 7.8886090522101181e-31f) L = 7.8886090522101181e-31f;
    if (L > 1.2676506002282294e30f) L = 1.2676506002282294e30f;
    inv = 1.0f / sqrtf(L);
    out[0] = v[0] * inv; out[1] = v[1] * inv; out[2] = v[2] * inv;
}

static float ref_log2(float x)
{
    uint32_t ue;
    float ef, m, s, s2, p;
    if (!(x >= 1.17549435e-38f)) return x >= 0.0f ? -INFINITY : bits(0x7FC00000u);
    ue = fbits(x) - 0x3F3504F3u;
    ef = (float)((int32_t)ue >> 23);
    m = bits((ue & 0x007FFFFFu) + 0x3F3504F3u);
    s = (m - 1.0f) * (1.0f / (m + 1.0f));
    s2 = s * s;
    p = fmaf(fmaf(fmaf(0.43174004554748535f, s2, 0.5767142176628113f), s2, 0.9617988467216492f), s2, 2.885390043258667f);
    return fmaf(s, p, ef);
}

static int ref_clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

/* fetch(k) */
static void ref_fetch(const ref_texture* t, uint32_t level, float u, float v, float out[4], uint64_t* n)
{
    uint32_t w = t->width, h = t->height, k;
    size_t off = 0;
    float tx, ty, fx, fy;
    int i0, j0, x0, x1, y0, y1, c;
    const uint8_t *p00, *p10, *p01, *p11;
    for (k = 0; k < level; ++k) { off += (size_t)w * h; w = w > 1u ? w >> 1 : 1u; h = h > 1u ? h >> 1 : 1u; }
    tx = fmaf(u, (float)w, -0.5f); ty = fmaf(v, (float)h, -0.5f);
    i0 = (int)floorf(tx); j0 = (int)floorf(ty);
    fx = tx - floorf(tx); fy = ty - floorf(ty);
    x0 = ref_clampi(i0, 0, (int)w - 1); x1 = ref_clampi(i0 + 1, 0, (int)w - 1);
    y0 = ref_clampi(j0, 0, (int)h - 1); y1 = ref_clampi(j0 + 1, 0, (int)h - 1);
    n[N_CLAMP_LEFT] += x0 != i0; n[N_CLAMP_RIGHT] += x1 != i0 + 1; n[N_CLAMP_TOP] += y0 != j0; n[N_CLAMP_BOTTOM] += y1 != j0 + 1;
    p00 = t->texels + 4u * (off + (size_t)y0 * w + (size_t)x0); p10 = t->texels + 4u * (off + (size_t)y0 * w + (size_t)x1);
    p01 = t->texels + 4u * (off + (size_t)y1 * w + (size_t)x0); p11 = t->texels + 4u * (off + (size_t)y1 * w + (size_t)x1);
    for (c = 0; c < 4; ++c) {
        const float top = ref_lerp((float)p00[c] / 255.0f, (float)p10[c] / 255.0f, fx);
        const float bot = ref_lerp((float)p01[c] / 255.0f, (float)p11[c] / 255.0f, fx);
        out[c] = ref_lerp(top, bot, fy);
    }
}

/* sample(T) */
static void ref_sample(const ref_texture* t, float u, float v, float s, float texelsPerUnit, float out[4], uint64_t* n)
{
    const uint32_t L = t->mipLevels > 1u ? t->mipLevels : 1u;
    float raw, lod, l0f, fl, a[4], b[4];
    uint32_t l0, l1;
    int c;
    if (L == 1u) { ++n[N_ONE_LEVEL]; ref_fetch(t, 0u, u, v, out, n); return; }
    raw = ref_log2(s * texelsPerUnit);
    lod = fminf(fmaxf(raw, 0.0f), (float)(L - 1u));
    if (!(raw > 0.0f)) ++n[N_LOD_LOW];
    else if (raw >= (float)(L - 1u)) ++n[N_LOD_HIGH];
    else ++n[N_LOD_INTERIOR];
    l0f = floorf(lod);
    fl = lod - l0f;
    l0 = (uint32_t)l0f;
    l1 = l0 + 1u < L - 1u ? l0 + 1u : L - 1u;
    ref_fetch(t, l0, u, v, a, n);
    ref_fetch(t, l1, u, v, b, n);
    for (c = 0; c < 4; ++c) out[c] = ref_lerp(a[c], b[c], fl);
}

static void ref_load(const void* plane, size_t idx, int isHalf, float out[4])
{
    int c;
    if (isHalf) { const uint16_t* p = (const uint16_t*)plane + 4u * idx; for (c = 0; c < 4; ++c) out[c] = decal_ref_h2f(p[c]); }
    else { const float* p = (const float*)plane + 4u * idx; for (c = 0; c < 4; ++c) out[c] = p[c]; }
}
static void ref_store(void* plane, size_t idx, int isHalf, int c, float value)
{
    if (isHalf) ((uint16_t*)plane)[4u * idx + (size_t)c] = decal_ref_f2h(value);
    else ((float*)plane)[4u * idx + (size_t)c] = value;
}

/* vz: View + 8 (four floats); proj5: Proj[5].  passed2: NULL, or W * H words that take, per pixel of the call's rows, the set of
 * decals d (bit d) the pixel passes step 2 of (whatever step 1 says). */
void decal_ref(const float* vz, float proj5, const uint32_t* depth, void* g0, void* g1, void* g2, uint32_t formatFlags, const ref_decal* decals,
               uint32_t nDecals, const ref_texture* textures, uint32_t nTextures, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint64_t* n,
               uint64_t* passed2)
{
    const int h0 = (formatFlags & 0x1000u) != 0, h1 = (formatFlags & 0x2000u) != 0, h2 = (formatFlags & 0x4000u) != 0;
    const float pix = 2.0f / (proj5 * (float)H);
    uint32_t px, py, d;
    int c;
    for (py = row0; py < row0 + rows; ++py)
        for (px = 0; px < W; ++px) {
            const size_t idx = (size_t)py * W + px;
            float G0[4], G1[4], G2[4], n0[3], alb[3], nrm[3], rough, metal, s;
            uint32_t stored = 0;
            if (passed2) passed2[idx] = 0;
            if (!((depth[idx] & 0xFFFFFFu) < 0xFFFFFFu)) { ++n[N_UNCOVERED]; continue; }
            ref_load(g0, idx, h0, G0); ref_load(g1, idx, h1, G1); ref_load(g2, idx, h2, G2);
            ref_normalize3(G2, n0);
            for (c = 0; c < 3; ++c) { alb[c] = G1[c]; nrm[c] = n0[c]; }
            rough = G1[3]; metal = G0[3];
            s = ref_mulcol1(G0, vz) * pix;
            if (!(fabsf(G0[0]) < INFINITY && fabsf(G0[1]) < INFINITY && fabsf(G0[2]) < INFINITY)) ++n[N_NONFINITE_POSITION];
            for (d = 0; d < nDecals; ++d) {
                const ref_decal* D = decals + d;
                float q[3], fade, u, v, t[4], a;
                int in2 = 1, in3 = 1, mapped;
                for (c = 0; c < 3; ++c) in2 = in2 && G0[c] >= D->boundsMin[c] && G0[c] <= D->boundsMax[c];
                if (passed2 && in2) passed2[idx] |= 1ull << d;
                if (D->texture >= nTextures) { ++n[N_BAD_TEXTURE]; continue; }                    /* step 1 */
                if (!in2) { ++n[N_OUTSIDE_BOUNDS]; continue; }                                      /* step 2 */
                for (c = 0; c < 3; ++c) { q[c] = ref_mulcol1(G0, D->invWorld + 4 * c); in3 = in3 && fabsf(q[c]) <= 0.5f; }
                if (!in3) { ++n[N_OUTSIDE_BOX]; continue; }                                         /* step 3 */
                fade = ref_saturate(fmaf(ref_dot3(n0, D->normalW), D->fadeScale, D->fadeBias));     /* step 4 */
                if (fade == 0.0f) ++n[N_FADE_ZERO]; else if (fade == 1.0f) ++n[N_FADE_ONE]; else ++n[N_FADE_PARTIAL];
                u = q[0] + 0.5f; v = 0.5f - q[1];                                                   /* step 5 */
                ref_sample(textures + D->texture, u, v, s, D->texelsPerUnit, t, n);                 /* step 6 */
                a = (t[3] * D->opacity) * fade;                                                     /* step 7 */
                if (!(a > 0.0f)) { ++n[N_A_NOT_POSITIVE]; continue; }
                if (D->flags & 1u) for (c = 0; c < 3; ++c) alb[c] = ref_lerp(alb[c], t[c] * D->tint[c], a);      /* step 8 */
                if (D->flags & 2u) rough = ref_lerp(rough, D->roughness, a);
                if (D->flags & 4u) metal = ref_lerp(metal, D->metalness, a);
                mapped = (D->flags & 8u) && D->normalTexture < nTextures;
                if ((D->flags & 8u) && !mapped) ++n[N_NORMAL_NO_MAP];
                if (mapped) {                                                                       /* step 9 */
                    float m[4], e[3];
                    ref_sample(textures + D->normalTexture, u, v, s, D->texelsPerUnit, m, n);
                    for (c = 0; c < 3; ++c) e[c] = fmaf(m[c], 2.0f, -1.0f);
                    for (c = 0; c < 3; ++c) {
                        const float wv = fmaf(e[2], D->normalW[c], fmaf(e[1], D->bitangentW[c], e[0] * D->tangentW[c]));
                        nrm[c] = ref_lerp(nrm[c], wv, a);
                    }
                }
                stored |= (D->flags & 7u) | (mapped ? 8u : 0u);
            }
            if (stored & 1u) { ++n[N_STORE_ALBEDO]; for (c = 0; c < 3; ++c) ref_store(g1, idx, h1, c, alb[c]); }
            if (stored & 2u) { ++n[N_STORE_ROUGHNESS]; ref_store(g1, idx, h1, 3, rough); }
            if (stored & 4u) { ++n[N_STORE_METALNESS]; ref_store(g0, idx, h0, 3, metal); }
            if (stored & 8u) { ++n[N_STORE_NORMAL]; for (c = 0; c < 3; ++c) ref_store(g2, idx, h2, c, nrm[c]); }
        }
}
