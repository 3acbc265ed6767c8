/* dof_ref.c -- the checker of crychic_dof (TEST INFRASTRUCTURE ONLY): plain C written from the definition in include/crychic_hip.h,
 * step by step, with its own restatement of the D24 decode.  It includes nothing of csrc/ and shares no code with the kernel: every
 * pixel walks the whole square of offsets, tests the disc, the frame and the depth order per tap, and divides at the end.  Built with
 * -ffp-contract=off: a product and a sum are fused exactly where fmaf is written.
 * It counts the branches of the definition it takes (COUNTERS in tests/dof_lib.py, in this order). */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { N_TAP_OUTSIDE, N_BEHIND, N_NOT_BEHIND, N_K_ZERO, N_K_INTERIOR, N_K_SIXTEEN, N_CE_BELOW_16, N_CE_IN_INV, N_C_ZERO, N_C_INTERIOR, N_C_HI, N_CLAMP_NAN,
       N_COUNTERS };

static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static float ref_d24(uint32_t u)
{
    const float v = (float)(u & 0xFFFFFFu);
    return fmaf(v, bits(0x33800001u), v * bits(0xA77FFFFFu));
}

static uint32_t ref_isqrt(uint32_t v)
{
    uint32_t r = (uint32_t)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1u) * (r + 1u) <= v) ++r;
    return r;
}

/* the number of offsets of the disc of radius R, and the largest channel sum they can give */
uint32_t dof_ref_disc(uint32_t R)
{
    uint32_t n = 0;
    int ox, oy;
    for (oy = -(int)R; oy <= (int)R; ++oy)
        for (ox = -(int)R; ox <= (int)R; ++ox) n += (uint32_t)(ox * ox + oy * oy) <= R * R;
    return n;
}
uint32_t dof_ref_inv(uint32_t c)
{
    const uint32_t m = c > 16u ? c : 16u;
    return (1u << 20) / (m * m);
}
uint32_t dof_ref_d16(int ox, int oy) { return ref_isqrt(256u * (uint32_t)(ox * ox + oy * oy)); }

/* consts: { A, B, focusDistance, aperture } as float bits */
uint32_t dof_ref_coc(const uint32_t* consts, uint32_t R, uint32_t depthWord, uint64_t* n)
{
    const float A = bits(consts[0]), B = bits(consts[1]), focusDistance = bits(consts[2]), aperture = bits(consts[3]);
    const float g = focusDistance / B;
    const float ap16 = aperture * 16.0f;
    const float hi = (float)(16u * R);
    const float d = ref_d24(depthWord);
    const float x = (d - A) * g;
    const float e = fabsf(1.0f - x);
    const float u = e * ap16;
    float v;
    uint32_t c;
    if (u != u) { v = 0.0f; if (n) n[N_CLAMP_NAN]++; }      /* fmaxf(NaN, 0) = 0 */
    else v = u < 0.0f ? 0.0f : (u > hi ? hi : u);
    c = (uint32_t)(v + 0.5f);
    if (n) n[c == 0u ? N_C_ZERO : (c == 16u * R ? N_C_HI : N_C_INTERIOR)]++;
    return c;
}

/* counters may be NULL.  coc (may be NULL): c of every texel of the frame, W * H uint32. */
void dof_ref(const uint32_t* consts, uint32_t R, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
             uint32_t rows, uint64_t* counters, uint32_t* coc)
{
    uint64_t n[N_COUNTERS] = { 0 };
    uint32_t px, py;
    int ox, oy, k;
    for (py = row0; py < row0 + rows; ++py)
        for (px = 0; px < W; ++px) {
            const size_t at = (size_t)py * W + px;
            const uint32_t Dp = depth[at] & 0xFFFFFFu;
            const uint32_t cp = dof_ref_coc(consts, R, depth[at], n);
            uint32_t sw = 0, sum[3] = { 0, 0, 0 };
            if (coc) coc[at] = cp;
            for (oy = -(int)R; oy <= (int)R; ++oy)
                for (ox = -(int)R; ox <= (int)R; ++ox) {
                    const int sx = (int)px + ox, sy = (int)py + oy;
                    size_t sat;
                    uint32_t Ds, cs, ce, w;
                    int kk;
                    if ((uint32_t)(ox * ox + oy * oy) > R * R) continue;
                    if (sx < 0 || sx >= (int)W || sy < 0 || sy >= (int)H) { n[N_TAP_OUTSIDE]++; continue; }
                    sat = (size_t)sy * W + (size_t)sx;
                    Ds = depth[sat] & 0xFFFFFFu;
                    cs = dof_ref_coc(consts, R, depth[sat], NULL);
                    if (Ds > Dp) { ce = cs < cp ? cs : cp; n[N_BEHIND]++; }
                    else { ce = cs; n[N_NOT_BEHIND]++; }
                    kk = (int)ce + 8 - (int)dof_ref_d16(ox, oy);
                    if (kk <= 0) { kk = 0; n[N_K_ZERO]++; }
                    else if (kk >= 16) { kk = 16; n[N_K_SIXTEEN]++; }
                    else n[N_K_INTERIOR]++;
                    n[ce < 16u ? N_CE_BELOW_16 : N_CE_IN_INV]++;
                    w = (uint32_t)kk * dof_ref_inv(ce);
                    sw += w;
                    for (k = 0; k < 3; ++k) sum[k] += w * in[4 * sat + k];
                }
            for (k = 0; k < 3; ++k) out[4 * at + k] = (uint8_t)((sum[k] + (sw >> 1)) / sw);
            out[4 * at + 3] = in[4 * at + 3];
        }
    if (counters) for (k = 0; k < N_COUNTERS; ++k) counters[k] += n[k];
}
