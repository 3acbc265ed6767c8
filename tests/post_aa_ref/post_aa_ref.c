/* post_aa_ref.c -- the checker of crychic_antialias (TEST INFRASTRUCTURE ONLY): the definition in include/crychic_hip.h, written
 * pixel by pixel in plain C with clamped fetches from the frame -- no tiles, no apron, none of the kernel's code.  Besides the
 * frame it returns how often each branch of the definition was taken. */
#include <stdint.h>
#include <string.h>

enum {
    AA_EARLY_COPY, AA_HORIZONTAL, AA_VERTICAL, AA_SIDE_A, AA_SIDE_B, AA_NEG_HIT, AA_NEG_K, AA_POS_HIT, AA_POS_K, AA_EDGE_WINS,
    AA_SUBPIX_WINS, AA_ZERO_WEIGHT, AA_COUNTERS
};

typedef struct aa_params { uint32_t absMin, relShift, searchSteps, subpix; } aa_params;

typedef struct frame { const uint8_t* px; int W, H; } frame;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static const uint8_t* texel(const frame* f, int x, int y) { return f->px + 4 * ((size_t)clampi(y, 0, f->H - 1) * (size_t)f->W + (size_t)clampi(x, 0, f->W - 1)); }
static int64_t luma(const frame* f, int x, int y)
{
    const uint8_t* t = texel(f, x, y);
    return 77 * (int64_t)t[0] + 150 * (int64_t)t[1] + 29 * (int64_t)t[2];
}
static int64_t absl(int64_t v) { return v < 0 ? -v : v; }
static int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }
static int64_t min2(int64_t a, int64_t b) { return a < b ? a : b; }

/* one direction of step 4: sign = -1 or +1; returns the distance, *end = the last delta */
static int search(const frame* f, int x, int y, int horizontal, int side, int sign, int K, int64_t Lp, int64_t g, int64_t* end, int* hit)
{
    *hit = 0;
    for (int i = 1; i <= K; ++i) {
        const int qx = horizontal ? x + sign * i : x, qy = horizontal ? y : y + sign * i;
        const int rx = horizontal ? qx : qx + side, ry = horizontal ? qy + side : qy;
        *end = luma(f, qx, qy) + luma(f, rx, ry) - Lp;
        if (2 * absl(*end) >= g) { *hit = 1; return i; }
    }
    return K;
}

/* rows [row0, row0 + rows) of out from in (both W x H RGBA8); counters: AA_COUNTERS sums over the pixels of those rows (added to) */
void aa_ref(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const aa_params* p, uint64_t* counters)
{
    const frame f = { in, (int)W, (int)H };
    for (int y = (int)row0; y < (int)(row0 + rows); ++y)
        for (int x = 0; x < (int)W; ++x) {
            uint8_t* o = out + 4 * ((size_t)y * W + (size_t)x);
            const int64_t M = luma(&f, x, y), N = luma(&f, x, y - 1), S = luma(&f, x, y + 1), E = luma(&f, x + 1, y), Wl = luma(&f, x - 1, y);
            const int64_t NW = luma(&f, x - 1, y - 1), NE = luma(&f, x + 1, y - 1), SW = luma(&f, x - 1, y + 1), SE = luma(&f, x + 1, y + 1);
            const int64_t hi = max2(max2(max2(M, N), max2(S, E)), Wl), lo = min2(min2(min2(M, N), min2(S, E)), Wl);
            const int64_t range = hi - lo;
            if (range == 0 || range < max2((int64_t)p->absMin, hi >> p->relShift)) {
                memcpy(o, texel(&f, x, y), 4);
                counters[AA_EARLY_COPY]++;
                continue;
            }
            const int64_t horz = absl(NW - 2 * Wl + SW) + 2 * absl(N - 2 * M + S) + absl(NE - 2 * E + SE);
            const int64_t vert = absl(NW - 2 * N + NE) + 2 * absl(Wl - 2 * M + E) + absl(SW - 2 * S + SE);
            const int horizontal = horz >= vert;
            counters[horizontal ? AA_HORIZONTAL : AA_VERTICAL]++;
            const int64_t a = horizontal ? N : Wl, b = horizontal ? S : E;
            const int64_t gA = absl(a - M), gB = absl(b - M);
            const int sideA = gA >= gB;
            counters[sideA ? AA_SIDE_A : AA_SIDE_B]++;
            const int side = sideA ? -1 : 1;
            const int64_t g = max2(gA, gB), nb = sideA ? a : b, Lp = M + nb;
            int64_t en = 0, ep = 0;
            int hitN, hitP;
            const int dn = search(&f, x, y, horizontal, side, -1, (int)p->searchSteps, Lp, g, &en, &hitN);
            const int dp = search(&f, x, y, horizontal, side, +1, (int)p->searchSteps, Lp, g, &ep, &hitP);
            counters[hitN ? AA_NEG_HIT : AA_NEG_K]++;
            counters[hitP ? AA_POS_HIT : AA_POS_K]++;
            const int dmin = dn <= dp ? dn : dp;
            const int64_t e = dn <= dp ? en : ep;
            int64_t wE = 0;
            if ((e < 0) != (M - nb < 0)) wE = 128 - (256 * dmin) / (dn + dp);
            const int64_t s = 2 * (N + S + E + Wl) + NW + NE + SW + SE;
            const int64_t t = absl(s - 12 * M);
            const int64_t r = min2(256, (256 * t) / (12 * range));
            const int64_t r2 = (r * r * (768 - 2 * r)) >> 16;
            const int64_t wS = (((r2 * r2) >> 8) * (int64_t)p->subpix) >> 8;
            const int64_t w = max2(wE, wS);
            if (wE > wS) counters[AA_EDGE_WINS]++;
            if (wS > wE) counters[AA_SUBPIX_WINS]++;
            if (w == 0) counters[AA_ZERO_WEIGHT]++;
            const uint8_t* c = texel(&f, x, y);
            const uint8_t* n = horizontal ? texel(&f, x, y + side) : texel(&f, x + side, y);
            for (int k = 0; k < 4; ++k) o[k] = (uint8_t)(((int64_t)c[k] * (256 - w) + (int64_t)n[k] * w + 128) >> 8);
        }
}
