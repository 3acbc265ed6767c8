// sharpen_core.hpp -- the body of crychic_sharpen (sharpen.hip), written so that a host compiler builds it too
// (tests/sharpen_host): one call per lane and phase, the caller supplies the exchange between neighbouring lanes.  The definition is
// the comment in include/crychic_hip.h; this file restates none of it beyond what the code needs.
//
// Structure: a streaming stencil without LDS.  The wide path (W a multiple of 4, both planes 16-byte aligned): a lane owns a quad --
// four pixels of a row, one 16-byte load and one 16-byte store -- and walks a strip of kSharpenStrip rows with the rows y - 1, y, y + 1
// in registers, so a strip of R rows reads R + 2.  The pixel left of a quad is the last pixel of the lane below, the pixel right of it
// the first of the lane above (sharpen_exchange_*: the kernel moves them with two lane permutes, the host harness through an array);
// lanes 0 and 63 of a wavefront read theirs with one 4-byte load (sharpen_load_row), and at the frame's edges the clamp makes it the
// quad's own pixel.  Lanes past the last quad of a partly filled wavefront load the last quad again, so that every lane of the
// wavefront reaches the permutes, and store nothing.  The narrow path: a lane per pixel, five 4-byte loads.
//
// Arithmetic: the two kinds of floor division go through binary32 with a reciprocal that may be off by one unit in the last place
// (v_rcp_f32 on the device, 1 / d on the host), and still give the floor:
//   sharpen_q12: floor(4096 n / d), n <= d <= 255.  The ratio fl(n r) carries a relative error below 1.5 * 2^-23, 7.4e-4 after the
//     scale by 4096; the exact quotient is an integer or at least 1 / 255 = 3.9e-3 away from one, so adding 1 / 512 and truncating gives
//     the floor.  It is monotone in the ratio: the smallest of the six quotients of a pixel is sharpen_q12 of the smallest ratio.
//   sharpen_div: floor(n / D), n <= 2^20 + 2^11, 512 <= D <= 4096.  trunc((n + 1/2) r) in one fma: the exact (n + 1/2) / D lies at least
//     1 / (2 D) from every integer, the reciprocal's error moves it by less than (n / D) * 1.5 * 2^-23 <= 0.19 / D and the fma's rounding
//     by less than 0.13 / D.  The definition's (num + den / 2) / den with den = 4 D is floor(((num + 2 D) >> 2) / D): a floor of a floor.
// tests/test_sharpen_host.py holds both to the integer division over every operand pair, with the reciprocal as it is and one unit
// either way.
#pragma once
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kSharpenMaxStrength = 256u;
constexpr uint32_t kSharpenMaxLimit = 3584u;            // Q12: 4 w <= 0.875, so the denominator 1 - 4 w stays at or above 1 / 8
constexpr uint32_t kSharpenThreads = 256u;              // four wavefronts side by side
constexpr uint32_t kSharpenStrip = 8u;                  // rows a lane walks
constexpr uint32_t kSharpenWave = 64u;

struct SharpenParams { uint32_t strength, limit, reserved[2]; };     // crychic_sharpen_params

struct SharpenArgs {
    const uint32_t* in;         // the frame's first pixel
    uint32_t* out;
    uint32_t W, H, row0, rows;
    uint32_t strength, limit;
    uint32_t groupsX;           // wide: workgroups across a row; the grid is groupsX * strips, one-dimensional
};

typedef uint32_t SharpenPx4 __attribute__((ext_vector_type(4)));

CRY_HD float sharpen_rcp(float d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(d);
#else
    return 1.0f / d;
#endif
}

CRY_HD uint32_t sharpen_q12(float ratio) { return (uint32_t)fma(ratio, 4096.0f, 0.001953125f); }
CRY_HD uint32_t sharpen_div(uint32_t n, float r) { return (uint32_t)fma((float)n, r, 0.5f * r); }      // r: the reciprocal of D

CRY_HD uint32_t sharpen_min3(uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a < b ? a : b; return m < c ? m : c; }
CRY_HD uint32_t sharpen_max3(uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a > b ? a : b; return m > c ? m : c; }

// The smaller of the two ratios one channel allows: mn / mx and (255 - mx) / (255 - mn), a denominator of 0 (then the numerator is 0
// too) counted as 1.
CRY_HD float sharpen_channel_ratio(uint32_t b, uint32_t d, uint32_t e, uint32_t f, uint32_t h)
{
    const uint32_t mn = sharpen_min3(sharpen_min3(b, d, e), f, h), mx = sharpen_max3(sharpen_max3(b, d, e), f, h);
    const uint32_t hiN = 255u - mx, hiD = 255u - mn;
    const float lo = (float)mn * sharpen_rcp((float)(mx ? mx : 1u));
    const float hi = (float)hiN * sharpen_rcp((float)(hiD ? hiD : 1u));
    return __builtin_fminf(lo, hi);
}

CRY_HD uint32_t sharpen_channel(uint32_t px, uint32_t c) { return (px >> (8u * c)) & 255u; }

// One pixel `e` from its cross.
CRY_HD uint32_t sharpen_pixel(uint32_t b, uint32_t d, uint32_t e, uint32_t f, uint32_t h, uint32_t strength, uint32_t limit)
{
    float ratio = 1.0f;
    for (uint32_t c = 0; c < 3u; ++c)
        ratio = __builtin_fminf(ratio, sharpen_channel_ratio(sharpen_channel(b, c), sharpen_channel(d, c), sharpen_channel(e, c), sharpen_channel(f, c),
                                                             sharpen_channel(h, c)));
    const uint32_t q = sharpen_q12(ratio);
    const uint32_t a = q < limit ? q : limit;
    const uint32_t t = mul24(a, strength) >> 8;
    const uint32_t D = 4096u - t;
    const float r = sharpen_rcp((float)D);
    uint32_t out = e & 0xFF000000u;
    for (uint32_t c = 0; c < 3u; ++c) {
        const uint32_t S = sharpen_channel(b, c) + sharpen_channel(d, c) + sharpen_channel(f, c) + sharpen_channel(h, c);
        const uint32_t num = (sharpen_channel(e, c) << 14) - mul24(t, S);        // never below 0: the limiter's promise
        out |= sharpen_div((num + 2u * D) >> 2, r) << (8u * c);
    }
    return out;
}

// ---- the wide path ------------------------------------------------------------------------------------------------------------------
// What a lane knows of itself: lane l of wavefront w of workgroup g along the row owns the quad at pixel 4 (256 g + 64 w + l).
struct SharpenLane {
    uint32_t x0;                // the first pixel of the quad it loads: its own, or the row's last quad where it has none
    uint32_t lane;              // 0 .. 63
    bool stores;                // it owns a quad
    bool rightmost;             // its quad ends the row: the pixel right of it is its own last
    uint32_t edgeX;             // the one more pixel it loads of every row (sharpen_load_row)
    uint32_t y0, y1;            // its strip: rows [y0, y1)
};

CRY_HD SharpenLane sharpen_lane(const SharpenArgs& a, uint32_t group, uint32_t thread)
{
    SharpenLane L;
    const uint32_t gx = group % a.groupsX, gy = group / a.groupsX;
    const uint32_t own = 4u * (gx * kSharpenThreads + thread);
    L.stores = own < a.W;
    L.x0 = L.stores ? own : a.W - 4u;
    L.lane = thread & (kSharpenWave - 1u);
    L.rightmost = L.x0 + 4u >= a.W;
    const uint32_t past = L.rightmost ? a.W - 1u : L.x0 + 4u, before = L.x0 ? L.x0 - 1u : 0u;
    L.edgeX = L.lane == 0u ? before : (L.lane == kSharpenWave - 1u ? past : L.x0);
    L.y0 = a.row0 + gy * kSharpenStrip;
    const uint32_t end = a.row0 + a.rows;
    L.y1 = L.y0 + kSharpenStrip < end ? L.y0 + kSharpenStrip : end;
    return L;
}

// A whole wavefront without a quad has nothing to do: the quad of its lane 0 lies past the row.
CRY_HD bool sharpen_wave_idle(const SharpenArgs& a, uint32_t group, uint32_t thread)
{
    return 4u * ((group % a.groupsX) * kSharpenThreads + (thread & ~(kSharpenWave - 1u))) >= a.W;
}

struct SharpenRow { SharpenPx4 px; uint32_t left, right; };

// Row y (clamped to the frame by the caller) of the lane's quad, and one more pixel: for lane 0 the one left of the quad, for lane 63
// the one right of it, clamped to the row, into both left and right.  Every other lane reads its own first pixel there -- a load
// without a branch around it, so that nothing waits for it before the row is used -- and has left and right filled by the exchange.
CRY_HD SharpenRow sharpen_load_row(const SharpenArgs& a, const SharpenLane& L, uint32_t y)
{
    SharpenRow R;
    const uint32_t* row = a.in + (size_t)y * a.W;
    R.px = *reinterpret_cast<const SharpenPx4*>(row + L.x0);
    R.left = R.right = row[L.edgeX];
    return R;
}

// What a lane hands to the lane above (its last pixel) and to the lane below (its first), and what it makes of what it is handed.
CRY_HD uint32_t sharpen_exchange_up(const SharpenRow& R) { return R.px[3]; }
CRY_HD uint32_t sharpen_exchange_down(const SharpenRow& R) { return R.px[0]; }
CRY_HD void sharpen_exchange_take(const SharpenLane& L, SharpenRow& R, uint32_t fromBelow, uint32_t fromAbove)
{
    if (L.lane != 0u) R.left = fromBelow;
    if (L.rightmost) R.right = R.px[3];
    else if (L.lane != kSharpenWave - 1u) R.right = fromAbove;
}

// Row `mid` of the quad from the rows above and below it.
CRY_HD SharpenPx4 sharpen_quad(const SharpenArgs& a, const SharpenPx4& up, const SharpenRow& mid, const SharpenPx4& dn)
{
    SharpenPx4 o;
    o[0] = sharpen_pixel(up[0], mid.left, mid.px[0], mid.px[1], dn[0], a.strength, a.limit);
    o[1] = sharpen_pixel(up[1], mid.px[0], mid.px[1], mid.px[2], dn[1], a.strength, a.limit);
    o[2] = sharpen_pixel(up[2], mid.px[1], mid.px[2], mid.px[3], dn[2], a.strength, a.limit);
    o[3] = sharpen_pixel(up[3], mid.px[2], mid.px[3], mid.right, dn[3], a.strength, a.limit);
    return o;
}

CRY_HD void sharpen_store(const SharpenArgs& a, const SharpenLane& L, uint32_t y, const SharpenPx4& v)
{
    if (L.stores) *reinterpret_cast<SharpenPx4*>(a.out + (size_t)y * a.W + L.x0) = v;
}

CRY_HD uint32_t sharpen_row_above(uint32_t y) { return y ? y - 1u : 0u; }
CRY_HD uint32_t sharpen_row_below(const SharpenArgs& a, uint32_t y) { return y + 1u < a.H ? y + 1u : a.H - 1u; }

// ---- the narrow path: pixel i of the row range, five loads ----------------------------------------------------------------------------
CRY_HD void sharpen_narrow(const SharpenArgs& a, uint32_t i)
{
    const uint32_t y = a.row0 + i / a.W, x = i % a.W;
    const uint32_t* row = a.in + (size_t)y * a.W;
    const uint32_t b = a.in[(size_t)sharpen_row_above(y) * a.W + x], h = a.in[(size_t)sharpen_row_below(a, y) * a.W + x];
    const uint32_t d = row[x ? x - 1u : 0u], f = row[x + 1u < a.W ? x + 1u : a.W - 1u];
    a.out[(size_t)y * a.W + x] = sharpen_pixel(b, d, row[x], f, h, a.strength, a.limit);
}

// The launch plan (sharpen.hip's launcher and the host harness walk it).
struct SharpenLaunch { SharpenArgs args; uint32_t groups; bool wide; };
CRY_HD SharpenLaunch sharpen_launch(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t strength, uint32_t limit)
{
    SharpenLaunch L;
    L.args.in = reinterpret_cast<const uint32_t*>(in);
    L.args.out = reinterpret_cast<uint32_t*>(out);
    L.args.W = W; L.args.H = H; L.args.row0 = row0; L.args.rows = rows;
    L.args.strength = strength; L.args.limit = limit;
    L.wide = (W & 3u) == 0u && (((uintptr_t)in | (uintptr_t)out) & 15u) == 0u;
    if (L.wide) {
        L.args.groupsX = (W / 4u + kSharpenThreads - 1u) / kSharpenThreads;
        L.groups = L.args.groupsX * ((rows + kSharpenStrip - 1u) / kSharpenStrip);      // at most 2^28 / 4 quads: far below 2^31
    } else {
        L.args.groupsX = 1u;
        L.groups = (rows * W + kSharpenThreads - 1u) / kSharpenThreads;                 // rows * W <= 2^28
    }
    return L;
}

}  // namespace cry
