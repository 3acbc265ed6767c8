/* sharpen_ref.c -- the checker of crychic_sharpen (TEST INFRASTRUCTURE ONLY): plain C written from the definition in
 * include/crychic_hip.h, with none of the kernel's code.  Every division is C's integer division of non-negative operands, which
 * is the floor.  Rows [row0, row0 + rows) of `out`; no other byte is written. */
#include <stddef.h>
#include <stdint.h>

static uint32_t clampi(int64_t v, int64_t hi) { return (uint32_t)(v < 0 ? 0 : (v > hi ? hi : v)); }

void sharpen_ref(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t strength, uint32_t limit)
{
    for (uint32_t y = row0; y < row0 + rows; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint8_t* e = in + 4u * ((size_t)y * W + x);
            const uint8_t* b = in + 4u * ((size_t)clampi((int64_t)y - 1, (int64_t)H - 1) * W + x);
            const uint8_t* h = in + 4u * ((size_t)clampi((int64_t)y + 1, (int64_t)H - 1) * W + x);
            const uint8_t* d = in + 4u * ((size_t)y * W + clampi((int64_t)x - 1, (int64_t)W - 1));
            const uint8_t* f = in + 4u * ((size_t)y * W + clampi((int64_t)x + 1, (int64_t)W - 1));
            uint32_t a = limit;
            for (int c = 0; c < 3; ++c) {
                uint32_t mn = e[c], mx = e[c];
                const uint8_t ring[4] = { b[c], d[c], f[c], h[c] };
                for (int k = 0; k < 4; ++k) {
                    if (ring[k] < mn) mn = ring[k];
                    if (ring[k] > mx) mx = ring[k];
                }
                const uint32_t lo = mx == 0u ? 0u : (mn << 12) / mx;
                const uint32_t hi = mn == 255u ? 0u : ((255u - mx) << 12) / (255u - mn);
                const uint32_t q = lo < hi ? lo : hi;
                if (q < a) a = q;
            }
            const uint32_t t = (a * strength) >> 8;
            const int32_t den = 4 * (4096 - (int32_t)t);
            uint8_t* o = out + 4u * ((size_t)y * W + x);
            for (int c = 0; c < 3; ++c) {
                const int32_t S = (int32_t)b[c] + d[c] + f[c] + h[c];
                const int32_t num = 16384 * (int32_t)e[c] - (int32_t)t * S;
                o[c] = (uint8_t)((num + den / 2) / den);        /* the definition has no clamp: num >= 0 and the quotient <= 255 */
            }
            o[3] = e[3];
        }
}
