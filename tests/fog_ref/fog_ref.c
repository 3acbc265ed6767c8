/* fog_ref.c -- the checker of crychic_fog (TEST INFRASTRUCTURE ONLY): plain C written from the definition in include/crychic_hip.h,
 * step by step, with its own restatement of the float primitives (IEEE 1.0f / x and sqrtf with the stated clamps, fmaf, the exp2
 * recurrence from the definition's constants).  It includes nothing of csrc/ and shares no code with the kernel.  Built with
 * -ffp-contract=off: a product and a sum are fused exactly where fmaf is written.
 * It counts the branches of the definition it takes (FOG_COUNTERS in tests/fog_lib.py, in this order). */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { N_CASCADE0, N_CASCADE1, N_CASCADE2, N_CASCADE3, N_BEYOND, N_OUTSIDE, N_LIT, N_SHADOWED, N_LC_L, N_LC_MAX, N_QI_ONE, N_QI_ZERO, N_QI_BETWEEN,
       N_CLAMPED, N_MIXED_RUN, N_COUNTERS };

static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static float ref_rcp(float b)
{
    if (b != b) return b;
    if (fabsf(b) < 1.17549435e-38f) return copysignf(INFINITY, b);      /* below 2^-126 */
    if (fabsf(b) > 8.50705917e37f) return copysignf(0.0f, b);           /* above 2^126 */
    return 1.0f / b;
}

static float ref_len_from_sq(float x)
{
    const float lo = 7.8886090522101181e-31f, hi = 1.2676506002282294e30f;      /* 2^-100, 2^100 */
    if (x != x) x = lo;
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return sqrtf(x);
}

static float ref_dot3(const float* u, const float* v) { return fmaf(u[2], v[2], fmaf(u[1], v[1], u[0] * v[0])); }
static float ref_mulcol(float x, float y, float z, float w, const float* m) { return fmaf(w, m[3], fmaf(z, m[2], fmaf(y, m[1], x * m[0]))); }
static float ref_mulcol1(float x, float y, float z, const float* m) { return fmaf(z, m[2], fmaf(y, m[1], x * m[0])) + m[3]; }

static float ref_d24(uint32_t u)
{
    const float v = (float)(u & 0xFFFFFFu);
    return fmaf(v, bits(0x33800001u), v * bits(0xA77FFFFFu));
}

static float ref_exp2(float z)
{
    static const float k[7] = { 0.00015406982856802642f, 0.0013400138122960925f, 0.009618260897696018f, 0.05550328269600868f,
                                0.24022649228572845f, 0.6931471824645996f, 1.0f };
    float n, f, p;
    int i;
    if (z != z) return z;
    if (z < -125.0f) z = -125.0f;
    if (z > 127.0f) z = 127.0f;
    n = rintf(z);                       /* the default rounding mode: to nearest, ties to even */
    f = z - n;
    p = k[0];
    for (i = 1; i < 7; ++i) p = fmaf(p, f, k[i]);
    return ldexpf(p, (int)n);
}

static const uint8_t BAYER[4][4] = { { 0, 8, 2, 10 }, { 12, 4, 14, 6 }, { 3, 11, 1, 9 }, { 15, 7, 13, 5 } };

/* params: { density bits, maxDistance bits, steps, ambient R G B, sun R G B } as nine uint32.  jitter == 0: jit = 0.5 for every pixel
 * (tests/fog_quality.py; never the definition).  counters may be NULL.  sums (may be NULL): S of every pixel of the rows, W * H uint32. */
void fog_ref(const float* invViewProj, const float* eye, const float* shadowTransforms /* [4][16] */, const uint32_t* depth,
             const uint32_t* const* maps, uint32_t dim, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
             const uint32_t* params, int jitter, uint64_t* counters, uint32_t* sums)
{
    const float density = bits(params[0]), maxDistance = bits(params[1]);
    const uint32_t N = params[2];
    const float invN = 1.0f / (float)N;
    const float c = -(density * 1.44269504f) * invN;
    const float sx = 2.0f / (float)W, sy = 2.0f / (float)H;
    const float dimf = (float)dim;
    float a[4][3];
    uint64_t n[N_COUNTERS] = { 0 };
    uint32_t px, py, i;
    int j, k;
    for (j = 0; j < 4; ++j)
        for (k = 0; k < 3; ++k) a[j][k] = ref_mulcol1(eye[0], eye[1], eye[2], shadowTransforms + 16 * j + 4 * k);
    for (py = row0; py < row0 + rows; ++py) {
        uint32_t runLit = 0, runShadowed = 0;        /* over the current run of 64 pixels of the row */
        for (px = 0; px < W; ++px) {
            const size_t at = (size_t)py * W + px;
            const float d = ref_d24(depth[at]);
            const float nx = fmaf((float)px + 0.5f, sx, -1.0f);
            const float ny = fmaf((float)py + 0.5f, -sy, 1.0f);
            float h[4], r[3], rw, L, Lc, invL, q, stepLen, jit;
            uint32_t qi, T = 65536u, S = 0u, Tend;
            for (k = 0; k < 4; ++k) h[k] = ref_mulcol(nx, ny, d, 1.0f, invViewProj + 4 * k);
            rw = ref_rcp(h[3]);
            for (k = 0; k < 3; ++k) r[k] = h[k] * rw - eye[k];
            L = ref_len_from_sq(ref_dot3(r, r));
            Lc = fminf(L, maxDistance);
            n[L <= maxDistance ? N_LC_L : N_LC_MAX]++;
            invL = ref_rcp(L);
            q = ref_exp2(c * Lc);
            qi = (uint32_t)fmaf(q, 65536.0f, 0.5f);
            n[qi == 65536u ? N_QI_ONE : (qi == 0u ? N_QI_ZERO : N_QI_BETWEEN)]++;
            stepLen = Lc * invN;
            jit = jitter ? ((float)BAYER[py & 3][px & 3] + 0.5f) / 16.0f : 0.5f;
            if ((px & 63u) == 0u) runLit = runShadowed = 0;
            for (i = 0; i < N; ++i) {
                const uint32_t Tn = (uint32_t)(((uint64_t)T * qi + 32768u) >> 16);
                const uint32_t w = T - Tn;
                const float t = ((float)i + jit) * stepLen;
                int lit = 1;
                if (t < 30.0f) j = 0; else if (t < 50.0f) j = 1; else if (t < 80.0f) j = 2; else if (t < 100.0f) j = 3; else j = 4;
                if (j == 4) n[N_BEYOND]++;
                else {
                    const float f = t * invL;
                    float s[3], fx, fy;
                    n[N_CASCADE0 + j]++;
                    for (k = 0; k < 3; ++k) {
                        const float* m = shadowTransforms + 16 * j + 4 * k;
                        const float b = fmaf(r[2], m[2], fmaf(r[1], m[1], r[0] * m[0]));
                        s[k] = fmaf(b, f, a[j][k]);
                    }
                    fx = s[0] * dimf;
                    fy = s[1] * dimf;
                    if (fx >= 0.0f && fx < dimf && fy >= 0.0f && fy < dimf) {
                        lit = s[2] <= ref_d24(maps[j][(size_t)(uint32_t)fy * dim + (uint32_t)fx]);
                        n[lit ? N_LIT : N_SHADOWED]++;
                        if (lit) runLit++; else runShadowed++;
                    } else n[N_OUTSIDE]++;
                }
                if (lit) S += w;
                T = Tn;
            }
            if (((px & 63u) == 63u || px == W - 1u) && runLit && runShadowed) n[N_MIXED_RUN]++;
            Tend = T;
            for (k = 0; k < 3; ++k) {
                const uint32_t o = ((uint32_t)in[4 * at + k] * Tend + params[3 + k] * (65536u - Tend) + params[6 + k] * S + 32768u) >> 16;
                if (o > 255u) n[N_CLAMPED]++;
                out[4 * at + k] = (uint8_t)(o < 255u ? o : 255u);
            }
            out[4 * at + 3] = in[4 * at + 3];
            if (sums) sums[at] = S;
        }
    }
    if (counters) for (k = 0; k < N_COUNTERS; ++k) counters[k] += n[k];
}
