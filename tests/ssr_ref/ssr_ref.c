/* ssr_ref.c -- the checker of crychic_ssr (TEST INFRASTRUCTURE ONLY): plain C written from the definition in include/crychic_hip.h,
 * step by step, with its own restatement of the float primitives (IEEE 1.0f / x and sqrtf with the stated clamps, fmaf).  It
 * includes nothing of csrc/ and shares no code with the kernel.  Built with -ffp-contract=off: a product and a sum are fused exactly
 * where fmaf is written.
 * It counts the branches of the definition it takes (COUNTERS in tests/ssr_lib.py, in this order) and can write a debug plane. */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { N_SKY, N_ROUGH, N_BEHIND_NEAR, N_NEAR_CLIPPED, N_OWN_SKIP, N_LEFT_FRAME, N_PAST_FAR, N_HIT_FIRST, N_HIT_LATER, N_THICK_REJECT, N_BIAS_REJECT,
       N_REFINE_MOVED, N_NO_HIT, N_EDGE_FADED, N_LENGTH_FADED, N_K_ZERO, N_COUNTERS };
/* the status word of the debug plane */
enum { ST_SKY, ST_ROUGH, ST_BEHIND_NEAR, ST_LEFT_FRAME, ST_PAST_FAR, ST_EXHAUSTED, ST_HIT };

static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static float ref_rcp(float b)
{
    if (b != b) return b;
    if (fabsf(b) < 1.17549435e-38f) return copysignf(INFINITY, b);      /* below 2^-126 */
    if (fabsf(b) > 8.50705917e37f) return copysignf(0.0f, b);           /* above 2^126 */
    return 1.0f / b;
}

static float ref_clamp_len2(float x)
{
    const float lo = 7.8886090522101181e-31f, hi = 1.2676506002282294e30f;      /* 2^-100, 2^100 */
    if (x != x) x = lo;
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return x;
}

static float ref_dot3(const float* u, const float* v) { return fmaf(u[2], v[2], fmaf(u[1], v[1], u[0] * v[0])); }
static float ref_mulcol(float x, float y, float z, float w, const float* m) { return fmaf(w, m[3], fmaf(z, m[2], fmaf(y, m[1], x * m[0]))); }

static void ref_normalize3(const float* v, float* o)
{
    const float inv = 1.0f / sqrtf(ref_clamp_len2(ref_dot3(v, v)));
    o[0] = v[0] * inv; o[1] = v[1] * inv; o[2] = v[2] * inv;
}

static float ref_d24(uint32_t u)
{
    const float v = (float)(u & 0xFFFFFFu);
    return fmaf(v, bits(0x33800001u), v * bits(0xA77FFFFFu));
}

static float ref_saturate(float x) { if (!(x > 0.0f)) return 0.0f; return x >= 1.0f ? 1.0f : x; }       /* a NaN gives 0 */

static const uint8_t BAYER[4][4] = { { 0, 8, 2, 10 }, { 12, 4, 14, 6 }, { 3, 11, 1, 9 }, { 15, 7, 13, 5 } };

typedef struct { float hw, hh, Wf, Hf, A, B, bias, thickness; float s0[3], ds[3]; uint32_t W, px, py; const uint32_t* depth; } ray_t;

static void screen(const ray_t* r, const float* h, float* s)
{
    const float rw = ref_rcp(h[3]);
    s[0] = fmaf(h[0] * rw, r->hw, r->hw);
    s[1] = fmaf(-(h[1] * rw), r->hh, r->hh);
    s[2] = h[2] * rw;
}

/* the sample at t: 0 outside the frame, 1 inside at or past the far plane, 2 ok (then *ix, *iy and *dr are set) */
static int sample(const ray_t* r, float t, uint32_t* ix, uint32_t* iy, float* dr)
{
    const float x = fmaf(r->ds[0], t, r->s0[0]), y = fmaf(r->ds[1], t, r->s0[1]);
    *dr = fmaf(r->ds[2], t, r->s0[2]);
    if (!(x >= 0.0f && x < r->Wf && y >= 0.0f && y < r->Hf)) return 0;
    if (!(*dr < 1.0f)) return 1;
    *ix = (uint32_t)x;
    *iy = (uint32_t)y;
    return 2;
}

/* step 5 on pixel (ix, iy): 1 a hit; 0 not; *why (may be NULL): 1 the thickness bound alone refused it, 2 the bias bound did */
static int hit_test(const ray_t* r, float dr, uint32_t ix, uint32_t iy, int* why)
{
    const uint32_t v = r->depth[(size_t)iy * r->W + ix] & 0xFFFFFFu;
    const float dz = ref_d24(v);
    const float D = (dr - r->A) * (dz - r->A);
    const float n = r->B * (dz - dr);
    if (why) *why = 0;
    if (v == 0xFFFFFFu || !(dr > dz)) return 0;
    if (!(r->bias * D <= n)) { if (why) *why = 2; return 0; }
    if (!(n <= r->thickness * D)) { if (why) *why = 1; return 0; }
    return 1;
}

/* g0, g1, g2: float4 planes.  params: the eight words of crychic_ssr_params.  counters and debug may be NULL; debug is W * H * 4 int32:
 * { status, hx, hy, tq } of every pixel of the rows (hx, hy, tq only with status ST_HIT). */
void ssr_ref(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, const float* nearZ, const float* g0,
             const float* g1, const float* g2, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
             uint32_t rows, const uint32_t* params, uint64_t* counters, int32_t* debug)
{
    const float maxDistance = bits(params[0]), thickness = bits(params[1]), bias = bits(params[2]), maxRoughness = bits(params[3]);
    const uint32_t N = params[4], E = params[5], intensity = params[6];
    const float sx = 2.0f / (float)W, sy = 2.0f / (float)H;
    const float invN = 1.0f / (float)N, wmin = *nearZ;
    uint64_t n[N_COUNTERS] = { 0 };
    uint32_t px, py, i;
    int k, c;
    ray_t r;
    r.Wf = (float)W; r.Hf = (float)H; r.hw = r.Wf * 0.5f; r.hh = r.Hf * 0.5f;
    r.A = proj[10]; r.B = proj[11]; r.bias = bias; r.thickness = thickness; r.W = W; r.depth = depth;
    for (py = row0; py < row0 + rows; ++py)
        for (px = 0; px < W; ++px) {
            const size_t at = (size_t)py * W + px;
            const uint32_t u = depth[at] & 0xFFFFFFu;
            const float rough = g1[4 * at + 3];
            int32_t* dbg = debug ? debug + 4 * at : NULL;
            float d, nx, ny, h[4], rw, P[3], PE[3], V[3], Nw[3], R[3], Q[3], h0[4], h1[4], s1[3], t2, jit, tHit = 0.0f, lo, hi;
            uint32_t hx = 0, hy = 0, ix, iy, I = 0;
            int found = 0, status = ST_EXHAUSTED;
            for (k = 0; k < 4; ++k) out[4 * at + k] = in[4 * at + k];
            if (u == 0xFFFFFFu) { n[N_SKY]++; if (dbg) dbg[0] = ST_SKY; continue; }
            if (!(rough < maxRoughness)) { n[N_ROUGH]++; if (dbg) dbg[0] = ST_ROUGH; continue; }
            /* step 2 */
            d = ref_d24(u);
            nx = fmaf((float)px + 0.5f, sx, -1.0f);
            ny = fmaf((float)py + 0.5f, -sy, 1.0f);
            for (k = 0; k < 4; ++k) h[k] = ref_mulcol(nx, ny, d, 1.0f, invViewProj + 4 * k);
            rw = ref_rcp(h[3]);
            for (k = 0; k < 3; ++k) { P[k] = h[k] * rw; PE[k] = P[k] - eye[k]; }
            ref_normalize3(PE, V);
            ref_normalize3(g2 + 4 * at, Nw);
            t2 = 2.0f * ref_dot3(Nw, V);
            for (k = 0; k < 3; ++k) { R[k] = fmaf(-t2, Nw[k], V[k]); Q[k] = fmaf(R[k], maxDistance, P[k]); }
            /* step 3 */
            for (k = 0; k < 4; ++k) { h0[k] = ref_mulcol(P[0], P[1], P[2], 1.0f, viewProj + 4 * k); h1[k] = ref_mulcol(Q[0], Q[1], Q[2], 1.0f, viewProj + 4 * k); }
            if (!(h0[3] > wmin)) { n[N_BEHIND_NEAR]++; if (dbg) dbg[0] = ST_BEHIND_NEAR; continue; }
            if (h1[3] < wmin) {
                const float tt = (h0[3] - wmin) * ref_rcp(h0[3] - h1[3]);
                const float md = maxDistance * tt;
                n[N_NEAR_CLIPPED]++;
                for (k = 0; k < 3; ++k) Q[k] = fmaf(R[k], md, P[k]);
                for (k = 0; k < 4; ++k) h1[k] = ref_mulcol(Q[0], Q[1], Q[2], 1.0f, viewProj + 4 * k);
            }
            screen(&r, h0, r.s0);
            screen(&r, h1, s1);
            for (k = 0; k < 3; ++k) r.ds[k] = s1[k] - r.s0[k];
            /* steps 4 and 5 */
            jit = ((float)BAYER[py & 3][px & 3] + 0.5f) / 16.0f;
            for (i = 0; i < N && !found; ++i) {
                const float t = ((float)i + jit) * invN;
                float dr;
                int why;
                const int s = sample(&r, t, &ix, &iy, &dr);
                if (s == 0) { n[N_LEFT_FRAME]++; status = ST_LEFT_FRAME; break; }
                if (s == 1) { n[N_PAST_FAR]++; status = ST_PAST_FAR; break; }
                if (ix == px && iy == py) { n[N_OWN_SKIP]++; continue; }
                if (hit_test(&r, dr, ix, iy, &why)) { found = 1; I = i; tHit = t; hx = ix; hy = iy; }
                else if (why == 1) n[N_THICK_REJECT]++;
                else if (why == 2) n[N_BIAS_REJECT]++;
            }
            if (!found) { n[N_NO_HIT]++; if (dbg) dbg[0] = status; continue; }
            n[I == 0 ? N_HIT_FIRST : N_HIT_LATER]++;
            /* step 6 */
            lo = (I == 0) ? 0.0f : ((float)(I - 1) + jit) * invN;
            hi = tHit;
            for (k = 0; k < 4; ++k) {       /* CRYCHIC_SSR_REFINE */
                const float tm = (lo + hi) * 0.5f;
                float dr;
                if (sample(&r, tm, &ix, &iy, &dr) == 2 && !(ix == px && iy == py) && hit_test(&r, dr, ix, iy, NULL)) { hi = tm; hx = ix; hy = iy; }
                else lo = tm;
            }
            if (hi != tHit) n[N_REFINE_MOVED]++;
            tHit = hi;
            /* steps 7 to 9 */
            {
                const size_t ht = (size_t)hy * W + hx;
                const float f0 = 1.0f - ref_saturate(ref_dot3(Nw, R));
                const float f2 = f0 * f0;
                const float f5 = (f2 * f2) * f0;
                uint32_t e = hx, fe, tq, fd, allZero = 1;
                if (W - 1 - hx < e) e = W - 1 - hx;
                if (hy < e) e = hy;
                if (H - 1 - hy < e) e = H - 1 - hy;
                fe = (e < E ? e : E) * 65536u / E;
                tq = (uint32_t)(tHit * 65536.0f);
                fd = 4u * (65536u - tq);
                if (fd > 65536u) fd = 65536u;
                if (fe < 65536u) n[N_EDGE_FADED]++;
                if (fd < 65536u) n[N_LENGTH_FADED]++;
                for (c = 0; c < 3; ++c) {
                    const float albedo = g1[4 * at + c], metal = g0[4 * at + 3];
                    const float R0 = fmaf(metal, albedo - 0.04f, 0.04f);
                    float w = (1.0f - rough) * fmaf(1.0f - R0, f5, R0);
                    uint32_t wq, K;
                    w = fminf(fmaxf(w, 0.0f), 1.0f);        /* a NaN gives 0 */
                    wq = (uint32_t)fmaf(w, 65536.0f, 0.5f);
                    K = (uint32_t)(((uint64_t)wq * fe) >> 16);
                    K = (uint32_t)(((uint64_t)K * fd) >> 16);
                    K = (K * intensity) >> 8;
                    if (K) allZero = 0;
                    out[4 * at + c] = (uint8_t)(((uint32_t)in[4 * at + c] * (65536u - K) + (uint32_t)in[4 * ht + c] * K + 32768u) >> 16);
                }
                if (allZero) n[N_K_ZERO]++;
                if (dbg) { dbg[0] = ST_HIT; dbg[1] = (int32_t)hx; dbg[2] = (int32_t)hy; dbg[3] = (int32_t)tq; }
            }
        }
    if (counters) for (k = 0; k < N_COUNTERS; ++k) counters[k] += n[k];
}
