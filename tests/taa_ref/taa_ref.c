/* taa_ref.c -- the checker of crychic_taa (TEST INFRASTRUCTURE ONLY): plain C written from the definition in include/crychic_hip.h,
 * step by step, with its own restatement of the float primitives (IEEE 1.0f / x with the stated clamps, fmaf).  It includes nothing
 * of csrc/ and shares no code with the kernel.  Built with -ffp-contract=off: a product and a sum are fused exactly where fmaf is
 * written.  It records the branch of the definition each pixel takes (TAA_BRANCH_* in tests/taa_lib.py). */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { B_HISTORY = 1, B_FX = 2, B_FY = 4, B_CLAMPED = 8 };     /* bits of a pixel's branch byte */

static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static float ref_rcp(float b)
{
    if (b != b) return b;
    if (fabsf(b) < 1.17549435e-38f) return copysignf(INFINITY, b);      /* below 2^-126 */
    if (fabsf(b) > 8.50705917e37f) return copysignf(0.0f, b);           /* above 2^126 */
    return 1.0f / b;
}

static float ref_mulcol(float x, float y, float z, float w, const float* m) { return fmaf(w, m[3], fmaf(z, m[2], fmaf(y, m[1], x * m[0]))); }
static float ref_mulcol1(float x, float y, float z, const float* m) { return fmaf(z, m[2], fmaf(y, m[1], x * m[0])) + m[3]; }

static float ref_d24(uint32_t u)
{
    const float v = (float)(u & 0xFFFFFFu);
    return fmaf(v, bits(0x33800001u), v * bits(0xA77FFFFFu));
}

static uint32_t clampu(int64_t v, uint32_t hi) { return v < 0 ? 0u : (v > (int64_t)hi ? hi : (uint32_t)v); }

/* history planes: W * H * 4 uint16.  flags: 1 = RESET, 2 = NO_CLAMP.  branch (may be NULL): W * H bytes, the rows' pixels written. */
void taa_ref(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, const uint8_t* in,
             const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t blend,
             uint32_t flags, uint8_t* branch)
{
    const float sx = 2.0f / (float)W, sy = 2.0f / (float)H, hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    const float xmax = (float)((W - 1u) * 256u), ymax = (float)((H - 1u) * 256u);
    uint32_t px, py;
    int i, j, k;
    for (py = row0; py < row0 + rows; ++py)
        for (px = 0; px < W; ++px) {
            const size_t at = (size_t)py * W + px;
            const uint8_t* c = in + 4 * at;
            uint32_t lo[3] = { 65535u, 65535u, 65535u }, hi[3] = { 0u, 0u, 0u }, n[3];
            uint8_t br = 0;
            int history = 0;
            float fxp = 0.0f, fyp = 0.0f;
            /* step 1 */
            for (j = -1; j <= 1; ++j)
                for (i = -1; i <= 1; ++i) {
                    const uint8_t* t = in + 4 * ((size_t)clampu((int64_t)py + j, H - 1u) * W + clampu((int64_t)px + i, W - 1u));
                    for (k = 0; k < 3; ++k) {
                        const uint32_t v = 256u * t[k];
                        if (v < lo[k]) lo[k] = v;
                        if (v > hi[k]) hi[k] = v;
                    }
                }
            /* steps 2 .. 4 */
            {
                const float d = ref_d24(depth[at]);
                const float nx = fmaf((float)px + 0.5f, sx, -1.0f);
                const float ny = fmaf((float)py + 0.5f, -sy, 1.0f);
                float h[4], P[3], a[4], b[4], rw, ra, rb, vx, vy;
                for (k = 0; k < 4; ++k) h[k] = ref_mulcol(nx, ny, d, 1.0f, invViewProj + 4 * k);
                rw = ref_rcp(h[3]);
                for (k = 0; k < 3; ++k) P[k] = h[k] * rw;
                for (k = 0; k < 4; ++k) {
                    a[k] = ref_mulcol1(P[0], P[1], P[2], curViewProj + 4 * k);
                    b[k] = ref_mulcol1(P[0], P[1], P[2], prevViewProj + 4 * k);
                }
                ra = ref_rcp(a[3]);
                rb = ref_rcp(b[3]);
                vx = (a[0] * ra - b[0] * rb) * hw;
                vy = (b[1] * rb - a[1] * ra) * hh;
                fxp = ((float)px - vx) * 256.0f;
                fyp = ((float)py - vy) * 256.0f;
                history = !(flags & 1u) && b[3] > 0.0f && fxp >= 0.0f && fxp <= xmax && fyp >= 0.0f && fyp <= ymax;
            }
            if (history) {
                const int X = (int)floorf(fxp), Y = (int)floorf(fyp);
                const uint32_t xi = (uint32_t)(X >> 8), fx = (uint32_t)(X & 255), yi = (uint32_t)(Y >> 8), fy = (uint32_t)(Y & 255);
                const uint32_t x1 = xi + 1u < W - 1u ? xi + 1u : W - 1u, y1 = yi + 1u < H - 1u ? yi + 1u : H - 1u;
                const uint16_t* t00 = historyIn + 4 * ((size_t)yi * W + xi);
                const uint16_t* t10 = historyIn + 4 * ((size_t)yi * W + x1);
                const uint16_t* t01 = historyIn + 4 * ((size_t)y1 * W + xi);
                const uint16_t* t11 = historyIn + 4 * ((size_t)y1 * W + x1);
                br |= B_HISTORY | (fx ? B_FX : 0) | (fy ? B_FY : 0);
                for (k = 0; k < 3; ++k) {
                    const uint32_t top = (uint32_t)t00[k] * (256u - fx) + (uint32_t)t10[k] * fx;
                    const uint32_t bot = (uint32_t)t01[k] * (256u - fx) + (uint32_t)t11[k] * fx;
                    const uint32_t hv = (top * (256u - fy) + bot * fy + 32768u) >> 16;
                    uint32_t hc = hv;
                    if (!(flags & 2u)) {                 /* step 5 */
                        if (hc < lo[k]) hc = lo[k];
                        if (hc > hi[k]) hc = hi[k];
                        if (hc != hv) br |= B_CLAMPED;
                    }
                    n[k] = (hc * (256u - blend) + (uint32_t)c[k] * 256u * blend + 128u) >> 8;      /* step 6 */
                }
            } else
                for (k = 0; k < 3; ++k) n[k] = 256u * c[k];
            /* step 7 */
            for (k = 0; k < 3; ++k) {
                const uint32_t o = (n[k] + 128u) >> 8;
                historyOut[4 * at + k] = (uint16_t)n[k];
                out[4 * at + k] = (uint8_t)(o < 255u ? o : 255u);
            }
            historyOut[4 * at + 3] = (uint16_t)(256u * c[3]);
            out[4 * at + 3] = c[3];
            if (branch) branch[at] = br;
        }
}
