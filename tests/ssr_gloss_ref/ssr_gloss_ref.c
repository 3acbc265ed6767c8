/* ssr_gloss_ref.c -- the checker of crychic_ssr_pyramid and crychic_ssr_glossy (TEST INFRASTRUCTURE ONLY): plain C written from the
 * definition in include/crychic_hip.h, step by step, with its own restatement of the float primitives (IEEE 1.0f / x and sqrtf with
 * the stated clamps, fmaf, det_log2).  It includes nothing of csrc/ and shares no code with the kernels.  Built with
 * -ffp-contract=off: a product and a sum are fused exactly where fmaf is written.  Steps 1 to 9 are tests/ssr_ref's, restated here so
 * that the whole pass is covered; 6a and 6b are new.
 * It counts the branches of the definition it takes (COUNTERS in tests/ssr_gloss_lib.py, in this order) and can write a debug plane. */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { N_SKY, N_ROUGH, N_BEHIND_NEAR, N_NEAR_CLIPPED, N_OWN_SKIP, N_LEFT_FRAME, N_PAST_FAR, N_HIT_FIRST, N_HIT_LATER, N_THICK_REJECT, N_BIAS_REJECT,
       N_REFINE_MOVED, N_NO_HIT, N_EDGE_FADED, N_LENGTH_FADED, N_K_ZERO,
       N_LQ_ZERO, N_LQ_POSITIVE, N_F_ZERO, N_F_POSITIVE, N_K_NEFF, N_CLAMP_LEFT, N_CLAMP_RIGHT, N_CLAMP_TOP, N_CLAMP_BOTTOM, N_COUNTERS };
#define MAX_LEVELS 8    /* CRYCHIC_SSR_GLOSS_MAX_LEVELS */
/* the status word of the debug plane */
enum { ST_SKY, ST_ROUGH, ST_BEHIND_NEAR, ST_LEFT_FRAME, ST_PAST_FAR, ST_EXHAUSTED, ST_HIT };

static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

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

static float ref_len_from_sq(float x) { return sqrtf(ref_clamp_len2(x)); }

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

/* ---- the pyramid --------------------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t nEff, w[MAX_LEVELS], h[MAX_LEVELS]; size_t off[MAX_LEVELS], bytes; } plan_t;

static void make_plan(uint32_t W, uint32_t H, uint32_t levels, plan_t* p)
{
    size_t at = 0;
    uint32_t k = 0;
    memset(p, 0, sizeof *p);
    p->w[0] = W; p->h[0] = H;
    while (k + 1 < levels && !(p->w[k] == 1 && p->h[k] == 1)) {
        ++k;
        p->w[k] = (p->w[k - 1] + 1) >> 1;
        p->h[k] = (p->h[k - 1] + 1) >> 1;
        p->off[k] = at;
        p->bytes = at + (size_t)p->w[k] * p->h[k] * 4;
        at = (p->bytes + 15) & ~(size_t)15;
    }
    p->nEff = k;
}

/* n_eff, and with sizes != NULL the 3 words { W_k, H_k, offset in bytes } of level k = 0 .. MAX_LEVELS - 1, then the workspace's bytes */
uint32_t ssr_gloss_plan_ref(uint32_t W, uint32_t H, uint32_t levels, uint64_t* sizes)
{
    plan_t p;
    uint32_t k;
    make_plan(W, H, levels, &p);
    if (sizes) {
        for (k = 0; k < MAX_LEVELS; ++k) { sizes[3 * k] = p.w[k]; sizes[3 * k + 1] = p.h[k]; sizes[3 * k + 2] = p.off[k]; }
        sizes[3 * MAX_LEVELS] = p.bytes;
    }
    return p.nEff;
}

static long clampl(long v, long n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

/* levels 1 .. n_eff of `in`'s pyramid into `workspace` (only the levels' own bytes are written) */
void ssr_gloss_pyramid_ref(const uint8_t* in, uint32_t W, uint32_t H, uint32_t levels, uint8_t* workspace)
{
    static const uint32_t wgt[4] = { 1, 3, 3, 1 };
    plan_t p;
    uint32_t k, x, y, c, i, j;
    make_plan(W, H, levels, &p);
    for (k = 1; k <= p.nEff; ++k) {
        const uint8_t* src = k == 1 ? in : workspace + p.off[k - 1];
        uint8_t* dst = workspace + p.off[k];
        const uint32_t sw = p.w[k - 1], sh = p.h[k - 1];
        for (y = 0; y < p.h[k]; ++y)
            for (x = 0; x < p.w[k]; ++x)
                for (c = 0; c < 4; ++c) {
                    uint32_t sum = 0;
                    for (j = 0; j < 4; ++j)
                        for (i = 0; i < 4; ++i) {
                            const long xs = clampl(2L * x - 1 + i, sw), ys = clampl(2L * y - 1 + j, sh);
                            sum += wgt[i] * wgt[j] * src[4 * ((size_t)ys * sw + xs) + c];
                        }
                    dst[4 * ((size_t)y * p.w[k] + x) + c] = (uint8_t)((sum + 32) >> 6);
                }
    }
}

/* fetch(k) of step 6b for channel c */
static uint32_t fetch(const uint8_t* in, const uint8_t* pyramid, const plan_t* p, uint32_t k, uint32_t hx, uint32_t hy, uint32_t c, uint64_t* n)
{
    const uint8_t* lv = k == 0 ? in : pyramid + p->off[k];
    const uint32_t wk = p->w[k], hk = p->h[k];
    const uint32_t Tx = ((2 * hx + 1) * 128) >> k, Ty = ((2 * hy + 1) * 128) >> k;
    const uint32_t Ux = (Tx > 128 ? Tx : 128) - 128, Uy = (Ty > 128 ? Ty : 128) - 128;
    uint32_t x0 = Ux >> 8, y0 = Uy >> 8, x1, y1, top, bot;
    const uint32_t fx = Ux & 255, fy = Uy & 255;
    if (n && c == 0) {
        if (Tx < 128) n[N_CLAMP_LEFT]++;
        if (Ty < 128) n[N_CLAMP_TOP]++;
        if (x0 + 1 > wk - 1) n[N_CLAMP_RIGHT]++;
        if (y0 + 1 > hk - 1) n[N_CLAMP_BOTTOM]++;
    }
    if (x0 > wk - 1) x0 = wk - 1;
    if (y0 > hk - 1) y0 = hk - 1;
    x1 = x0 + 1 < wk - 1 ? x0 + 1 : wk - 1;
    y1 = y0 + 1 < hk - 1 ? y0 + 1 : hk - 1;
    top = lv[4 * ((size_t)y0 * wk + x0) + c] * (256 - fx) + lv[4 * ((size_t)y0 * wk + x1) + c] * fx;
    bot = lv[4 * ((size_t)y1 * wk + x0) + c] * (256 - fx) + lv[4 * ((size_t)y1 * wk + x1) + c] * fx;
    return (top * (256 - fy) + bot * fy + 32768) >> 16;
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

/* g0, g1, g2: float4 planes.  params: the eight words of crychic_ssr_params.  pyramid: what ssr_gloss_pyramid_ref left for `in` at
 * gloss[1] levels.  gloss: the four words of crychic_ssr_gloss_params.  counters and debug may be NULL; debug is W * H * 8 int32:
 * { status, hx, hy, tq, lq, R, G, B } of every pixel of the rows (all but status only with status ST_HIT; R, G, B the fetched hit). */
void ssr_gloss_ref(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, const float* nearZ, const float* g0,
             const float* g1, const float* g2, const uint32_t* depth, const uint8_t* in, const uint8_t* pyramid, uint8_t* out,
                   uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint32_t* params, const uint32_t* gloss, uint64_t* counters, int32_t* debug)
{
    const float coneScale = bits(gloss[0]);
    plan_t plan;
    const float maxDistance = bits(params[0]), thickness = bits(params[1]), bias = bits(params[2]), maxRoughness = bits(params[3]);
    const uint32_t N = params[4], E = params[5], intensity = params[6];
    const float sx = 2.0f / (float)W, sy = 2.0f / (float)H;
    const float invN = 1.0f / (float)N, wmin = *nearZ;
    uint64_t n[N_COUNTERS] = { 0 };
    uint32_t px, py, i;
    int k, c;
    ray_t r;
    make_plan(W, H, gloss[1], &plan);
    r.Wf = (float)W; r.Hf = (float)H; r.hw = r.Wf * 0.5f; r.hh = r.Hf * 0.5f;
    r.A = proj[10]; r.B = proj[11]; r.bias = bias; r.thickness = thickness; r.W = W; r.depth = depth;
    for (py = row0; py < row0 + rows; ++py)
        for (px = 0; px < W; ++px) {
            const size_t at = (size_t)py * W + px;
            const uint32_t u = depth[at] & 0xFFFFFFu;
            const float rough = g1[4 * at + 3];
            int32_t* dbg = debug ? debug + 8 * at : NULL;
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
                /* step 6a */
                const float dxs = (float)hx - (float)px, dys = (float)hy - (float)py;
                const float Lpx = ref_len_from_sq(fmaf(dxs, dxs, dys * dys));
                const float rc = (coneScale * rough) * Lpx;
                float lam = rc > 1.0f ? ref_log2(rc) : 0.0f;
                uint32_t lq, kl, fl, hitc[3];
                if (!(lam < (float)plan.nEff)) lam = (float)plan.nEff;
                lq = (uint32_t)fmaf(lam, 256.0f, 0.5f);
                kl = lq >> 8; fl = lq & 255u;
                n[lq == 0 ? N_LQ_ZERO : N_LQ_POSITIVE]++;
                n[fl == 0 ? N_F_ZERO : N_F_POSITIVE]++;
                if (kl == plan.nEff) n[N_K_NEFF]++;
                /* step 6b */
                for (c = 0; c < 3; ++c) {
                    const uint32_t vk = fetch(in, pyramid, &plan, kl, hx, hy, (uint32_t)c, n);
                    hitc[c] = fl == 0 ? vk : (vk * (256 - fl) + fetch(in, pyramid, &plan, kl + 1, hx, hy, (uint32_t)c, n) * fl + 128) >> 8;
                }
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
                    out[4 * at + c] = (uint8_t)(((uint32_t)in[4 * at + c] * (65536u - K) + hitc[c] * K + 32768u) >> 16);
                }
                if (allZero) n[N_K_ZERO]++;
                if (dbg) { dbg[0] = ST_HIT; dbg[1] = (int32_t)hx; dbg[2] = (int32_t)hy; dbg[3] = (int32_t)tq; dbg[4] = (int32_t)lq;
                           dbg[5] = (int32_t)hitc[0]; dbg[6] = (int32_t)hitc[1]; dbg[7] = (int32_t)hitc[2]; }
            }
        }
    if (counters) for (k = 0; k < N_COUNTERS; ++k) counters[k] += n[k];
}
