/* bloom_ref.c -- the checker of crychic_bloom (TEST INFRASTRUCTURE ONLY): plain C written from the definition in
 * include/crychic_hip.h, step by step.  It includes nothing of csrc/ and shares no code with the kernels: every level is a plain
 * array of uint16_t[4] of its own, every destination texel walks its 16 source texels with both coordinates clamped, the weight is
 * an integer division, and the unwind writes new arrays instead of running in place.
 * It counts the branches of the definition it takes (COUNTERS in tests/bloom_lib.py, in this order). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { N_W_ZERO, N_W_INTERIOR, N_W_FULL, N_CLAMP_DOWN, N_CLAMP_UP, N_SATURATED, N_COUNTERS };
#define MAX_LEVELS 8

static uint64_t* g_n;

/* n_eff = min(n, max(1, ceil(log2(max(W, H))))) */
uint32_t bloom_ref_levels(uint32_t W, uint32_t H, uint32_t n)
{
    const uint32_t m = W > H ? W : H;
    uint32_t lg = 0;
    uint64_t p = 1;
    while (p < m) { p *= 2; ++lg; }
    if (lg < 1) lg = 1;
    return n < lg ? n : lg;
}

/* the size of level k: W_k = (W_(k-1) + 1) >> 1 */
void bloom_ref_size(uint32_t W, uint32_t H, uint32_t k, uint32_t* w, uint32_t* h)
{
    while (k--) { W = (W + 1) >> 1; H = (H + 1) >> 1; }
    *w = W; *h = H;
}

static uint32_t clamp_to(int64_t v, uint32_t n, int counter)
{
    if (v < 0) { g_n[counter]++; return 0; }
    if (v > (int64_t)n - 1) { g_n[counter]++; return n - 1; }
    return (uint32_t)v;
}

/* D_(k+1) from a source level of sw x sh texels (uint16_t[4] each) */
static void down(const uint16_t* src, uint32_t sw, uint32_t sh, uint16_t* dst)
{
    static const uint32_t tap[4] = { 1, 3, 3, 1 };
    const uint32_t dw = (sw + 1) >> 1, dh = (sh + 1) >> 1;
    uint32_t x, y, ch;
    int i, j;
    for (y = 0; y < dh; ++y)
        for (x = 0; x < dw; ++x) {
            uint32_t sum[3] = { 0, 0, 0 };
            for (j = 0; j < 4; ++j)
                for (i = 0; i < 4; ++i) {
                    const uint32_t sx = clamp_to(2 * (int64_t)x - 1 + i, sw, N_CLAMP_DOWN), sy = clamp_to(2 * (int64_t)y - 1 + j, sh, N_CLAMP_DOWN);
                    for (ch = 0; ch < 3; ++ch) sum[ch] += tap[i] * tap[j] * src[((size_t)sy * sw + sx) * 4 + ch];
                }
            for (ch = 0; ch < 3; ++ch) dst[((size_t)y * dw + x) * 4 + ch] = (uint16_t)((sum[ch] + 32) >> 6);
            dst[((size_t)y * dw + x) * 4 + 3] = 0;
        }
}

/* up(S)(x, y) for one channel */
static uint32_t up(const uint16_t* S, uint32_t sw, uint32_t sh, uint32_t x, uint32_t y, uint32_t ch)
{
    const int64_t xc = x >> 1, yc = y >> 1;
    const uint32_t xn = clamp_to((x & 1) ? xc + 1 : xc - 1, sw, N_CLAMP_UP), yn = clamp_to((y & 1) ? yc + 1 : yc - 1, sh, N_CLAMP_UP);
    const uint32_t a = S[((size_t)yc * sw + xc) * 4 + ch], b = S[((size_t)yc * sw + xn) * 4 + ch];
    const uint32_t c = S[((size_t)yn * sw + xc) * 4 + ch], d = S[((size_t)yn * sw + xn) * 4 + ch];
    return (9 * a + 3 * b + 3 * c + d + 8) >> 4;
}

/* params: { T, K, r, I, n }.  in, out: W x H RGBA8; rows [row0, row0 + rows) of out are written.  levels[k - 1], k = 1 .. n_eff: where
 * U_k goes (W_k x H_k x 4 uint16_t), or NULL; downs[k - 1] likewise for D_k.  counters: N_COUNTERS sums, added to.  Returns n_eff. */
uint32_t bloom_ref(const uint32_t* params, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                   uint16_t* const* levels, uint16_t* const* downs, uint64_t* counters)
{
    const uint32_t T = params[0], K = params[1], r = params[2], I = params[3], n = params[4];
    const uint32_t nEff = bloom_ref_levels(W, H, n);
    uint16_t* D[MAX_LEVELS + 1];
    uint16_t* U[MAX_LEVELS + 1];
    uint32_t w[MAX_LEVELS + 1], h[MAX_LEVELS + 1];
    uint32_t k, x, y, ch;
    g_n = counters;
    for (k = 0; k <= nEff; ++k) {
        bloom_ref_size(W, H, k, &w[k], &h[k]);
        D[k] = (uint16_t*)malloc((size_t)w[k] * h[k] * 8);
        U[k] = (uint16_t*)malloc((size_t)w[k] * h[k] * 8);
    }
    /* level 0: the bright values */
    for (y = 0; y < H; ++y)
        for (x = 0; x < W; ++x) {
            const uint8_t* p = in + ((size_t)y * W + x) * 4;
            const uint32_t L = 77u * p[0] + 150u * p[1] + 29u * p[2];
            uint32_t wt = 0;
            if (L > 256 * T) {
                wt = (L - 256 * T) / K;
                if (wt > 256) wt = 256;
            }
            g_n[wt == 0 ? N_W_ZERO : (wt == 256 ? N_W_FULL : N_W_INTERIOR)]++;
            for (ch = 0; ch < 3; ++ch) D[0][((size_t)y * W + x) * 4 + ch] = (uint16_t)(p[ch] * wt);
            D[0][((size_t)y * W + x) * 4 + 3] = 0;
        }
    for (k = 1; k <= nEff; ++k) down(D[k - 1], w[k - 1], h[k - 1], D[k]);
    memcpy(U[nEff], D[nEff], (size_t)w[nEff] * h[nEff] * 8);
    for (k = nEff - 1; k >= 1; --k)
        for (y = 0; y < h[k]; ++y)
            for (x = 0; x < w[k]; ++x) {
                const size_t at = ((size_t)y * w[k] + x) * 4;
                for (ch = 0; ch < 3; ++ch) U[k][at + ch] = (uint16_t)((D[k][at + ch] * (256 - r) + up(U[k + 1], w[k + 1], h[k + 1], x, y, ch) * r + 128) >> 8);
                U[k][at + 3] = 0;
            }
    for (y = row0; y < row0 + rows; ++y)
        for (x = 0; x < W; ++x) {
            const size_t at = ((size_t)y * W + x) * 4;
            for (ch = 0; ch < 3; ++ch) {
                const uint32_t v = in[at + ch] + ((up(U[1], w[1], h[1], x, y, ch) * I + 32768) >> 16);
                if (v > 255) g_n[N_SATURATED]++;
                out[at + ch] = (uint8_t)(v > 255 ? 255 : v);
            }
            out[at + 3] = in[at + 3];
        }
    for (k = 1; k <= nEff; ++k) {
        if (levels && levels[k - 1]) memcpy(levels[k - 1], U[k], (size_t)w[k] * h[k] * 8);
        if (downs && downs[k - 1]) memcpy(downs[k - 1], D[k], (size_t)w[k] * h[k] * 8);
    }
    for (k = 0; k <= nEff; ++k) { free(D[k]); free(U[k]); }
    return nEff;
}
