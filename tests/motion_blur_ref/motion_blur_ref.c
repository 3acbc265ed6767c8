/* motion_blur_ref.c -- the checker of crychic_motion_blur (TEST INFRASTRUCTURE ONLY): plain C written from the definition in
 * include/crychic_hip.h, step by step, with its own restatement of the float primitives (IEEE 1.0f / x with the stated clamps, fmaf)
 * and 64-bit integer arithmetic with real divisions.  It includes nothing of csrc/ and shares no code with the kernels.  Built with
 * -ffp-contract=off: a product and a sum are fused exactly where fmaf is written.  It records the branch of the definition each pixel
 * takes (B_* in tests/motion_blur_lib.py). */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { B_STILL = 1, B_CLAMPED = 2, B_INVALID = 4, B_FRONT = 8, B_BACK = 16 };     /* bits of a pixel's branch byte */

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

static int64_t floor_div(int64_t a, int64_t b) { int64_t q = a / b; if (a % b != 0 && ((a < 0) != (b < 0))) --q; return q; }
static int64_t iabs(int64_t v) { return v < 0 ? -v : v; }
static int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

static int64_t word_qx(uint32_t w) { return (int16_t)(uint16_t)(w & 0xFFFFu); }
static int64_t word_qy(uint32_t w) { return (int16_t)(uint16_t)(w >> 16); }
static int64_t word_len(uint32_t w) { const int64_t x = iabs(word_qx(w)), y = iabs(word_qy(w)); return x > y ? x : y; }
static uint64_t word_key(uint32_t w) { return ((uint64_t)word_len(w) << 32) | w; }

static uint32_t tiles_of(uint32_t n) { return (n + 15u) / 16u; }

static int64_t quantise(float s, int64_t R)
{
    return clampi((int64_t)floorf(fmaf(s, 16.0f, 0.5f)), -16 * R, 16 * R);
}

/* Steps A and A'.  workspace: W H 8 bytes of velocity texels, then the tile words.  branch (may be NULL): W H bytes, B_CLAMPED and
 * B_INVALID set here. */
void motion_blur_ref_velocity(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, uint32_t W,
                              uint32_t H, uint32_t shutter, uint32_t R, uint32_t* workspace, uint8_t* branch)
{
    const float sx = 2.0f / (float)W, sy = 2.0f / (float)H, hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    const float sh = (float)shutter * 0.00390625f, Rf = (float)R;
    uint32_t* tiles = workspace + 2 * (size_t)W * H;
    const uint32_t tilesX = tiles_of(W), tilesY = tiles_of(H);
    uint32_t px, py, tx, ty;
    int k;
    for (py = 0; py < H; ++py)
        for (px = 0; px < W; ++px) {
            const size_t at = (size_t)py * W + px;
            const float d = ref_d24(depth[at]);
            const float nx = fmaf((float)px + 0.5f, sx, -1.0f);
            const float ny = fmaf((float)py + 0.5f, -sy, 1.0f);
            float h[4], P[3], a[4], b[4], rw, ra, rb, vx, vy, s_x, s_y, m;
            uint8_t br = 0;
            int64_t qx, qy;
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
            if (!(a[3] > 0.0f && b[3] > 0.0f && fabsf(vx) < INFINITY && fabsf(vy) < INFINITY)) {
                vx = 0.0f;
                vy = 0.0f;
                br |= B_INVALID;
            }
            s_x = vx * sh;
            s_y = vy * sh;
            m = fabsf(s_x) > fabsf(s_y) ? fabsf(s_x) : fabsf(s_y);
            if (m > Rf) {
                const float kk = Rf * ref_rcp(m);
                s_x = s_x * kk;
                s_y = s_y * kk;
                br |= B_CLAMPED;
            }
            qx = quantise(s_x, R);
            qy = quantise(s_y, R);
            workspace[2 * at] = (uint32_t)(uint16_t)(int16_t)qx | ((uint32_t)(uint16_t)(int16_t)qy << 16);
            workspace[2 * at + 1] = depth[at] & 0xFFFFFFu;
            if (branch) branch[at] = br;
        }
    for (ty = 0; ty < tilesY; ++ty)
        for (tx = 0; tx < tilesX; ++tx) {
            uint64_t best = 0;
            int first = 1;
            for (py = 16 * ty; py < 16 * ty + 16 && py < H; ++py)
                for (px = 16 * tx; px < 16 * tx + 16 && px < W; ++px) {
                    const uint64_t key = word_key(workspace[2 * ((size_t)py * W + px)]);
                    if (first || key > best) best = key;
                    first = 0;
                }
            tiles[(size_t)ty * tilesX + tx] = (uint32_t)(best & 0xFFFFFFFFu);
        }
}

static const int kBayer[4][4] = { { 0, 8, 2, 10 }, { 12, 4, 14, 6 }, { 3, 11, 1, 9 }, { 15, 7, 13, 5 } };

/* Step B for rows [row0, row0 + rows).  branch (may be NULL): B_STILL, B_FRONT and B_BACK are ORed into the rows' bytes. */
void motion_blur_ref_gather(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t N,
                            const uint32_t* workspace, uint8_t* branch)
{
    const uint32_t* tiles = workspace + 2 * (size_t)W * H;
    const int64_t tilesX = tiles_of(W), tilesY = tiles_of(H);
    uint32_t px, py;
    int64_t i, j;
    int k;
    for (py = row0; py < row0 + rows; ++py)
        for (px = 0; px < W; ++px) {
            const size_t at = (size_t)py * W + px;
            const int64_t tx = px >> 4, ty = py >> 4;
            uint64_t best = 0;
            int first = 1;
            uint32_t vN;
            uint8_t br = 0;
            for (j = -1; j <= 1; ++j)
                for (i = -1; i <= 1; ++i) {
                    if (tx + i < 0 || tx + i >= tilesX || ty + j < 0 || ty + j >= tilesY) continue;
                    {
                        const uint64_t key = word_key(tiles[(ty + j) * tilesX + tx + i]);
                        if (first || key > best) best = key;
                        first = 0;
                    }
                }
            vN = (uint32_t)(best & 0xFFFFFFFFu);
            if (word_len(vN) < 8) {
                memcpy(out + 4 * at, in + 4 * at, 4);
                br |= B_STILL;
            } else {
                const int64_t nx = word_qx(vN), ny = word_qy(vN), b = kBayer[py & 3][px & 3];
                const uint32_t wordX = workspace[2 * at], dX = workspace[2 * at + 1];
                const int64_t lenX = word_len(wordX);
                int64_t Wt = 1, S[3];
                for (k = 0; k < 3; ++k) S[k] = in[4 * at + k];
                for (i = 0; i < (int64_t)N; ++i) {
                    const int64_t m = 16 * i + b - 8 * (int64_t)N;
                    const int64_t ox = floor_div(nx * m + 8 * (int64_t)N, 16 * (int64_t)N), oy = floor_div(ny * m + 8 * (int64_t)N, 16 * (int64_t)N);
                    const int64_t dist = iabs(ox) > iabs(oy) ? iabs(ox) : iabs(oy);
                    const int64_t sxp = clampi((int64_t)px + floor_div(ox + 8, 16), 0, (int64_t)W - 1);
                    const int64_t syp = clampi((int64_t)py + floor_div(oy + 8, 16), 0, (int64_t)H - 1);
                    const size_t sat = (size_t)syp * W + (size_t)sxp;
                    const uint32_t wordY = workspace[2 * sat], dY = workspace[2 * sat + 1];
                    const int64_t lenY = word_len(wordY);
                    const int front = dY <= dX && 2 * dist <= lenY, back = dY >= dX && 2 * dist <= lenX;
                    const int64_t w = front + back;
                    if (front) br |= B_FRONT;
                    if (back) br |= B_BACK;
                    Wt += w;
                    for (k = 0; k < 3; ++k) S[k] += w * in[4 * sat + k];
                }
                for (k = 0; k < 3; ++k) out[4 * at + k] = (uint8_t)floor_div(2 * S[k] + Wt, 2 * Wt);
                out[4 * at + 3] = in[4 * at + 3];
            }
            if (branch) branch[at] |= br;
        }
}
