/* taa_upscale_ref.c -- the checker of crychic_taa_upscale (TEST INFRASTRUCTURE ONLY): plain C written from the definition in
 * include/crychic_hip.h, step by step, with its own restatement of the float primitives (IEEE 1.0f / x with the stated clamps, fmaf).
 * It includes nothing of csrc/ and shares no code with the kernel.  Built with -ffp-contract=off: a product and a sum are fused
 * exactly where fmaf is written.  It records the branch of the definition each output pixel takes and the weight it gave the current
 * frame (tests/taa_upscale_lib.py). */
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

static int64_t clampi(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
static int64_t floor_shift8(int64_t v) { return v >= 0 ? v / 256 : -((-v + 255) / 256); }       /* floor(v / 256) */
static int64_t low8(int64_t v) { return v - 256 * floor_shift8(v); }                            /* v mod 256, 0 .. 255 */

static int64_t position(uint32_t o, uint32_t Ni, uint32_t No, int J)
{
    return (int64_t)(((2u * (uint64_t)o + 1u) * Ni * 256u) / (2u * (uint64_t)No)) + J - 128;
}

static uint32_t near_axis(int64_t f, uint32_t Ni, uint32_t No)      /* 256 - dX */
{
    const int64_t du = f < 256 - f ? f : 256 - f;
    int64_t dX = (du * No) / Ni;
    if (dX > 256) dX = 256;
    return (uint32_t)(256 - dX);
}

/* history planes: Wo * Ho * 4 uint16.  flags: 1 = RESET, 2 = NO_CLAMP.  branch, weight (may be NULL): Wo * Ho bytes / uint16, the
 * rows' pixels written. */
void taa_upscale_ref(const float* invViewProj, const float* curViewProj, const float* prevViewProj, float jx, float jy, const uint32_t* depth,
                     const uint8_t* in, uint32_t Wi, uint32_t Hi, const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t Wo,
                     uint32_t Ho, uint32_t row0, uint32_t rows, uint32_t blend, uint32_t flags, uint8_t* branch, uint16_t* weight)
{
    const float sx = 2.0f / (float)Wi, sy = 2.0f / (float)Hi, hw = 0.5f * (float)Wi, hh = 0.5f * (float)Hi;
    const float rx = (float)Wo / (float)Wi, ry = (float)Ho / (float)Hi;
    const float xmax = (float)((Wo - 1u) * 256u), ymax = (float)((Ho - 1u) * 256u);
    const int Jx = (int)floorf(fmaf(jx, 256.0f, 0.5f)), Jy = (int)floorf(fmaf(jy, 256.0f, 0.5f));
    uint32_t ox, oy;
    int i, j, k;
    for (oy = row0; oy < row0 + rows; ++oy)
        for (ox = 0; ox < Wo; ++ox) {
            const size_t at = (size_t)oy * Wo + ox;
            /* step 1 */
            const int64_t U = position(ox, Wi, Wo, Jx), V = position(oy, Hi, Ho, Jy);
            const int64_t ui = floor_shift8(U), vi = floor_shift8(V), fu = low8(U), fv = low8(V);
            const int64_t tx = clampi(floor_shift8(U + 128), (int64_t)Wi - 1), ty = clampi(floor_shift8(V + 128), (int64_t)Hi - 1);
            const int64_t x0 = clampi(ui, (int64_t)Wi - 1), x1 = clampi(ui + 1, (int64_t)Wi - 1);
            const int64_t y0 = clampi(vi, (int64_t)Hi - 1), y1 = clampi(vi + 1, (int64_t)Hi - 1);
            const uint8_t* t00 = in + 4 * ((size_t)y0 * Wi + x0);
            const uint8_t* t10 = in + 4 * ((size_t)y0 * Wi + x1);
            const uint8_t* t01 = in + 4 * ((size_t)y1 * Wi + x0);
            const uint8_t* t11 = in + 4 * ((size_t)y1 * Wi + x1);
            const uint8_t cA = in[4 * ((size_t)ty * Wi + tx) + 3];
            uint32_t c256[3], lo[3] = { 65535u, 65535u, 65535u }, hi[3] = { 0u, 0u, 0u }, n[3], conf, conf2, wgt;
            uint8_t br = 0;
            int history = 0;
            float fxp = 0.0f, fyp = 0.0f;
            /* step 2 */
            for (k = 0; k < 3; ++k) {
                const uint32_t top = (uint32_t)t00[k] * (uint32_t)(256 - fu) + (uint32_t)t10[k] * (uint32_t)fu;
                const uint32_t bot = (uint32_t)t01[k] * (uint32_t)(256 - fu) + (uint32_t)t11[k] * (uint32_t)fu;
                c256[k] = (top * (uint32_t)(256 - fv) + bot * (uint32_t)fv + 128u) >> 8;
            }
            /* step 3 */
            conf = (near_axis(fu, Wi, Wo) * near_axis(fv, Hi, Ho)) >> 8;
            conf2 = (conf * conf) >> 8;
            wgt = (blend * conf2) >> 8;
            if (wgt > 256u) wgt = 256u;
            /* step 4 */
            for (j = -1; j <= 1; ++j)
                for (i = -1; i <= 1; ++i) {
                    const uint8_t* t = in + 4 * ((size_t)clampi(ty + j, (int64_t)Hi - 1) * Wi + (size_t)clampi(tx + i, (int64_t)Wi - 1));
                    for (k = 0; k < 3; ++k) {
                        const uint32_t v = 256u * t[k];
                        if (v < lo[k]) lo[k] = v;
                        if (v > hi[k]) hi[k] = v;
                    }
                }
            /* step 5 */
            {
                const float d = ref_d24(depth[(size_t)ty * Wi + tx]);
                const float nx = fmaf((float)tx + 0.5f, sx, -1.0f);
                const float ny = fmaf((float)ty + 0.5f, -sy, 1.0f);
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
                fxp = ((float)ox - vx * rx) * 256.0f;
                fyp = ((float)oy - vy * ry) * 256.0f;
                history = !(flags & 1u) && b[3] > 0.0f && fxp >= 0.0f && fxp <= xmax && fyp >= 0.0f && fyp <= ymax;
            }
            if (history) {
                const int X = (int)floorf(fxp), Y = (int)floorf(fyp);
                const uint32_t xi = (uint32_t)(X >> 8), fx = (uint32_t)(X & 255), yi = (uint32_t)(Y >> 8), fy = (uint32_t)(Y & 255);
                const uint32_t xn = xi + 1u < Wo - 1u ? xi + 1u : Wo - 1u, yn = yi + 1u < Ho - 1u ? yi + 1u : Ho - 1u;
                const uint16_t* h00 = historyIn + 4 * ((size_t)yi * Wo + xi);
                const uint16_t* h10 = historyIn + 4 * ((size_t)yi * Wo + xn);
                const uint16_t* h01 = historyIn + 4 * ((size_t)yn * Wo + xi);
                const uint16_t* h11 = historyIn + 4 * ((size_t)yn * Wo + xn);
                br |= B_HISTORY | (fx ? B_FX : 0) | (fy ? B_FY : 0);
                for (k = 0; k < 3; ++k) {
                    const uint32_t top = (uint32_t)h00[k] * (256u - fx) + (uint32_t)h10[k] * fx;
                    const uint32_t bot = (uint32_t)h01[k] * (256u - fx) + (uint32_t)h11[k] * fx;
                    const uint32_t hv = (top * (256u - fy) + bot * fy + 32768u) >> 16;
                    uint32_t hc = hv;
                    if (!(flags & 2u)) {
                        if (hc < lo[k]) hc = lo[k];
                        if (hc > hi[k]) hc = hi[k];
                        if (hc != hv) br |= B_CLAMPED;
                    }
                    n[k] = (hc * (256u - wgt) + c256[k] * wgt + 128u) >> 8;      /* step 6 */
                }
            } else
                for (k = 0; k < 3; ++k) n[k] = c256[k];
            for (k = 0; k < 3; ++k) {
                const uint32_t o = (n[k] + 128u) >> 8;
                historyOut[4 * at + k] = (uint16_t)n[k];
                out[4 * at + k] = (uint8_t)(o < 255u ? o : 255u);
            }
            historyOut[4 * at + 3] = (uint16_t)(256u * cA);
            out[4 * at + 3] = cA;
            if (branch) branch[at] = br;
            if (weight) weight[at] = (uint16_t)wgt;
        }
}
