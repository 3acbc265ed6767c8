/* grade_ref.c -- the checker of crychic_grade (TEST INFRASTRUCTURE ONLY): plain C written from the definition in
 * include/crychic_hip.h, one texel at a time, with none of the kernel's code: divisions are divisions, the three fractions are sorted
 * as a list, and each channel is interpolated on its own. */
#include <stdint.h>
#include <stddef.h>

static uint32_t entry(const uint8_t* lut, uint32_t N, const uint32_t v[3], int c)
{
    return lut[4u * ((size_t)v[0] + (size_t)N * ((size_t)v[1] + (size_t)N * (size_t)v[2])) + (size_t)c];
}

/* rows [row0, row0 + rows) of out from in (both W x H RGBA8), through the table of size N; no other byte of out is written */
void grade_ref(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint8_t* lut, uint32_t N)
{
    (void)H;
    for (size_t t = (size_t)row0 * W; t < (size_t)(row0 + rows) * W; ++t) {
        uint32_t cell[3], f[3];
        int order[3] = { 0, 1, 2 };
        for (int a = 0; a < 3; ++a) {
            const uint32_t p = (uint32_t)in[4 * t + a] * (N - 1u);
            cell[a] = p / 255u;
            if (cell[a] > N - 2u) cell[a] = N - 2u;
            f[a] = p - 255u * cell[a];
        }
        /* the axes by falling fraction (a stable insertion sort: ties keep red before green before blue) */
        for (int i = 1; i < 3; ++i)
            for (int j = i; j > 0 && f[order[j]] > f[order[j - 1]]; --j) {
                const int s = order[j]; order[j] = order[j - 1]; order[j - 1] = s;
            }
        const uint32_t f1 = f[order[0]], f2 = f[order[1]], f3 = f[order[2]];
        uint32_t v0[3], v1[3], v2[3], v3[3];
        for (int a = 0; a < 3; ++a) { v0[a] = v1[a] = v2[a] = cell[a]; v3[a] = cell[a] + 1u; }
        v1[order[0]] += 1u;
        v2[order[0]] += 1u;
        v2[order[1]] += 1u;
        for (int c = 0; c < 3; ++c) {
            const uint32_t n = (255u - f1) * entry(lut, N, v0, c) + (f1 - f2) * entry(lut, N, v1, c) + (f2 - f3) * entry(lut, N, v2, c) +
                               f3 * entry(lut, N, v3, c) + 127u;
            out[4 * t + c] = (uint8_t)(n / 255u);
        }
        out[4 * t + 3] = in[4 * t + 3];
    }
}
