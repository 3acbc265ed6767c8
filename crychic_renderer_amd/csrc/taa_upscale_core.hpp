// taa_upscale_core.hpp -- the body of crychic_taa_upscale (include/crychic_hip.h states the definition), built
// for the device (taa_upscale.hip) and for the host (tests/taa_upscale_host).  One lane per OUTPUT pixel, an 8 x 8 output tile per
// wavefront, four tiles side by side per workgroup, as in taa_core.hpp.  Lanes share nothing: a lane reads the 3 x 3 input texels
// around its nearest texel straight from memory (the four texels of its bilinear sample are among the nine, so they are selected and
// not read again; a tile's window is at most 10 x 10 input texels, which its lanes' loads share through the caches: no LDS, no
// barrier), reprojects the nearest texel's world point and gathers its display-size history with 8-byte loads.
//
// The wave votes are those of taa_core.hpp, and each only skips work whose result is already known: no lane of the wave has history
// (nothing is gathered), and a tap whose weight is 0 in every lane is not read.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "taa_core.hpp"

namespace cry {

constexpr uint32_t kTaaUpscaleMaxRatio = 4u;

struct TaaUpscaleParams { uint32_t blend, flags, reserved[6]; };   // crychic_taa_upscale_params

// the kernel's arguments (kernarg segment: every field is wave-uniform)
struct TaaUpscaleArgs {
    const uint32_t* depth;      // Wi x Hi
    const uint32_t* in;         // Wi x Hi
    const void* historyIn;      // Wo x Ho, four uint16_t per texel; NULL only with kTaaReset
    void* historyOut;
    uint32_t* out;              // Wo x Ho
    uint32_t Wi, Hi, Wo, Ho, row0, rowEnd, tilesX, blend, flags;
    uint32_t narrow;            // both positions' numerators fit 32 bits
    uint32_t mWo, mHo, mWi, mHi;        // tu_magic of the four divisors
    int32_t Jx, Jy;             // the jitter in 1/256 input texel
    float ivp[16];              // InvViewProj of the frame's own constants
    float cur[3][4], prev[3][4];        // columns 0, 1 and 3 of the unjittered view-projections
    float sx, sy, hw, hh, rx, ry, xmax, ymax;
};

// n / d for any 32-bit n and a divisor known on the host, without the division: m = tu_magic(d) = floor((2^32 - 1) / d) lies in
// [2^32 / d - 1, 2^32 / d), so n m / 2^32 lies in (n / d - 1, n / d] and the estimate (n m) >> 32 is the quotient or one below it,
// which one remainder test settles.
inline uint32_t tu_magic(uint32_t d) { return 0xFFFFFFFFu / d; }
CRY_HD uint32_t tu_div(uint32_t n, uint32_t d, uint32_t m)
{
    const uint32_t q = (uint32_t)(((uint64_t)n * m) >> 32);
    return n - q * d >= d ? q + 1u : q;
}

struct TaaUpscaleLaunch { TaaUpscaleArgs args; uint32_t groups; };      // groups == 0: nothing to launch

// The launcher's plan and the host-side constants of the definition.  The caller has checked every argument (api.cpp).
inline TaaUpscaleLaunch taa_upscale_launch(const float* invViewProj, const float* curViewProj, const float* prevViewProj, float jx, float jy,
                                           const uint32_t* depth, const uint8_t* in, uint32_t Wi, uint32_t Hi, const uint16_t* historyIn,
                                           uint16_t* historyOut, uint8_t* out, uint32_t Wo, uint32_t Ho, uint32_t row0, uint32_t rows,
                                           const TaaUpscaleParams& p)
{
    TaaUpscaleLaunch L;
    TaaUpscaleArgs& a = L.args;
    a.depth = depth;
    a.in = reinterpret_cast<const uint32_t*>(in);
    a.historyIn = historyIn;
    a.historyOut = historyOut;
    a.out = reinterpret_cast<uint32_t*>(out);
    a.Wi = Wi; a.Hi = Hi; a.Wo = Wo; a.Ho = Ho; a.row0 = row0; a.rowEnd = row0 + rows; a.blend = p.blend; a.flags = p.flags;
    a.tilesX = (Wo + kTaaGroupW - 1u) / kTaaGroupW;
    // (2 o + 1) Ni 128 < 256 No Ni
    a.narrow = (uint64_t)Wo * Wi * 256u <= 0xFFFFFFFFull && (uint64_t)Ho * Hi * 256u <= 0xFFFFFFFFull;
    a.mWo = tu_magic(Wo); a.mHo = tu_magic(Ho); a.mWi = tu_magic(Wi); a.mHi = tu_magic(Hi);
    a.Jx = (int32_t)__builtin_floorf(__builtin_fmaf(jx, 256.0f, 0.5f));
    a.Jy = (int32_t)__builtin_floorf(__builtin_fmaf(jy, 256.0f, 0.5f));
    for (int k = 0; k < 16; ++k) a.ivp[k] = invViewProj[k];
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 4; ++k) {
            a.cur[c][k] = curViewProj[4 * (c == 2 ? 3 : c) + k];
            a.prev[c][k] = prevViewProj[4 * (c == 2 ? 3 : c) + k];
        }
    a.sx = 2.0f / (float)Wi;
    a.sy = 2.0f / (float)Hi;
    a.hw = 0.5f * (float)Wi;
    a.hh = 0.5f * (float)Hi;
    a.rx = (float)Wo / (float)Wi;
    a.ry = (float)Ho / (float)Hi;
    a.xmax = (float)((Wo - 1u) * 256u);
    a.ymax = (float)((Ho - 1u) * 256u);
    const uint64_t groups = (uint64_t)a.tilesX * ((rows + kTaaTile - 1u) / kTaaTile);      // below 2^27: fits
    L.groups = (uint32_t)groups;
    return L;
}

// step 1: the position of output pixel o in the input frame, in 1/256 texel.  ((2 o + 1) Ni 256) / (2 No) == ((2 o + 1) Ni 128) / No
CRY_HD int32_t tu_position(uint32_t o, uint32_t Ni, uint32_t No, uint32_t mNo, int32_t J, bool narrow)
{
    const uint32_t q = narrow ? tu_div((2u * o + 1u) * Ni * 128u, No, mNo) : (uint32_t)(((uint64_t)(2u * o + 1u) * Ni * 128u) / No);    // below 256 Ni <= 2^30
    return (int32_t)q + J - 128;
}

CRY_HD uint32_t tu_clamp(int32_t v, uint32_t last) { return v < 0 ? 0u : ((uint32_t)v > last ? last : (uint32_t)v); }

// step 3: one axis of the confidence, 256 - the distance to the nearest input sample in 1/256 display pixel
CRY_HD uint32_t tu_near(uint32_t f, uint32_t Ni, uint32_t No, uint32_t mNi)
{
    const uint32_t du = taa_min(f, 256u - f);                   // at most 128: du No below 2^30
    return 256u - taa_min(256u, tu_div(du * No, Ni, mNi));
}

// step 2's filter of one channel of four bytes: 8.8
CRY_HD uint32_t tu_bilinear(uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11, uint32_t fx, uint32_t fy)
{
    const uint32_t top = t00 * (256u - fx) + t10 * fx, bot = t01 * (256u - fx) + t11 * fx;
    return (top * (256u - fy) + bot * fy + 128u) >> 8;
}

// of three texels at columns (or rows) l, c, r the one at x, which is one of them
CRY_HD uint32_t tu_pick(uint32_t x, uint32_t l, uint32_t c, uint32_t tl, uint32_t tc, uint32_t tr) { return x == c ? tc : (x == l ? tl : tr); }

// One pixel of the output.  `any`: a vote over the lanes that run together (the device: the wavefront's active lanes; the host: the
// lane's own predicate).  It only skips work whose result would be what it already is; no result depends on it.
template <class Any>
CRY_HD void taa_upscale_pixel(const TaaUpscaleArgs& a, uint32_t ox, uint32_t oy, Any any)
{
    const uint32_t at = oy * a.Wo + ox;                        // below 2^28
    // step 1
    const int32_t U = tu_position(ox, a.Wi, a.Wo, a.mWo, a.Jx, a.narrow != 0u), V = tu_position(oy, a.Hi, a.Ho, a.mHo, a.Jy, a.narrow != 0u);
    const uint32_t fu = (uint32_t)(U & 255), fv = (uint32_t)(V & 255);
    const uint32_t xa = tu_clamp(U >> 8, a.Wi - 1u), xb = tu_clamp((U >> 8) + 1, a.Wi - 1u);
    const uint32_t ya = tu_clamp(V >> 8, a.Hi - 1u), yb = tu_clamp((V >> 8) + 1, a.Hi - 1u);
    const uint32_t tx = tu_clamp((U + 128) >> 8, a.Wi - 1u), ty = tu_clamp((V + 128) >> 8, a.Hi - 1u);
    // step 4's neighbourhood, clamped to the frame; the bilinear four are among the nine
    const uint32_t xl = tx ? tx - 1u : 0u, xr = tx + 1u < a.Wi ? tx + 1u : tx;
    const uint32_t yu = ty ? ty - 1u : 0u, yd = ty + 1u < a.Hi ? ty + 1u : ty;
    const uint32_t rowU = yu * a.Wi, rowC = ty * a.Wi, rowD = yd * a.Wi;
    const uint32_t nb[9] = { a.in[rowU + xl], a.in[rowU + tx], a.in[rowU + xr], a.in[rowC + xl], a.in[rowC + tx], a.in[rowC + xr],
                             a.in[rowD + xl], a.in[rowD + tx], a.in[rowD + xr] };
    const uint32_t rawDepth = a.depth[rowC + tx];
    uint32_t colA[3], colB[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        colA[j] = tu_pick(xa, xl, tx, nb[3 * j], nb[3 * j + 1], nb[3 * j + 2]);
        colB[j] = tu_pick(xb, xl, tx, nb[3 * j], nb[3 * j + 1], nb[3 * j + 2]);
    }
    const uint32_t t00 = tu_pick(ya, yu, ty, colA[0], colA[1], colA[2]), t10 = tu_pick(ya, yu, ty, colB[0], colB[1], colB[2]);
    const uint32_t t01 = tu_pick(yb, yu, ty, colA[0], colA[1], colA[2]), t11 = tu_pick(yb, yu, ty, colB[0], colB[1], colB[2]);
    uint32_t lo[3], hi[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t mn = 255u, mx = 0u;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const uint32_t v = (nb[i] >> (8 * k)) & 255u;
            mn = taa_min(mn, v);
            mx = taa_max(mx, v);
        }
        lo[k] = mn << 8;
        hi[k] = mx << 8;
        // step 2
        c[k] = tu_bilinear((t00 >> (8 * k)) & 255u, (t10 >> (8 * k)) & 255u, (t01 >> (8 * k)) & 255u, (t11 >> (8 * k)) & 255u, fu, fv);
    }
    const uint32_t alpha = nb[4] >> 24;
    // step 3
    const uint32_t conf = (tu_near(fu, a.Wi, a.Wo, a.mWi) * tu_near(fv, a.Hi, a.Ho, a.mHi)) >> 8;
    const uint32_t weight = taa_min(256u, (a.blend * ((conf * conf) >> 8)) >> 8);
    // step 5: the nearest texel's world point and its velocity in input pixels
    bool hist = false;
    float fxp = 0.0f, fyp = 0.0f;
    if (!(a.flags & kTaaReset)) {                               // wave-uniform
        const float d = d24_to_float(rawDepth);
        const float nx = fma((float)tx + 0.5f, a.sx, -1.0f);
        const float ny = fma((float)ty + 0.5f, -a.sy, 1.0f);
        const float hx = mulcol(nx, ny, d, 1.0f, a.ivp), hy = mulcol(nx, ny, d, 1.0f, a.ivp + 4), hz = mulcol(nx, ny, d, 1.0f, a.ivp + 8);
        const float rw = rcp(mulcol(nx, ny, d, 1.0f, a.ivp + 12));
        const float Px = hx * rw, Py = hy * rw, Pz = hz * rw;
        const float a0 = mulcol1(Px, Py, Pz, a.cur[0]), a1 = mulcol1(Px, Py, Pz, a.cur[1]), a3 = mulcol1(Px, Py, Pz, a.cur[2]);
        const float b0 = mulcol1(Px, Py, Pz, a.prev[0]), b1 = mulcol1(Px, Py, Pz, a.prev[1]), b3 = mulcol1(Px, Py, Pz, a.prev[2]);
        const float ra = rcp(a3), rb = rcp(b3);
        const float vx = (a0 * ra - b0 * rb) * a.hw;
        const float vy = (b1 * rb - a1 * ra) * a.hh;
        fxp = ((float)ox - vx * a.rx) * 256.0f;
        fyp = ((float)oy - vy * a.ry) * 256.0f;
        hist = b3 > 0.0f && fxp >= 0.0f && fxp <= a.xmax && fyp >= 0.0f && fyp <= a.ymax;
    }
    uint32_t n[3] = { c[0], c[1], c[2] };
    if (any(hist)) {
        // in range with history: below 2^30.  Without: texel 0, never used
        const uint32_t X = hist ? (uint32_t)(int)__builtin_floorf(fxp) : 0u, Y = hist ? (uint32_t)(int)__builtin_floorf(fyp) : 0u;
        const uint32_t xi = X >> 8, fx = X & 255u, yi = Y >> 8, fy = Y & 255u;
        const uint32_t x1 = xi + 1u < a.Wo ? xi + 1u : xi, y1 = yi + 1u < a.Ho ? yi + 1u : yi;
        const uint32_t r0 = mul24(yi, a.Wo), r1 = mul24(y1, a.Wo);         // rows below 2^22, texel indices below 2^28: byte offsets below 2^31
        const bool right = any(hist && fx != 0u), below = any(hist && fy != 0u);
        const TaaTexel zero = { 0u, 0u };
        const TaaTexel h00 = load_at<TaaTexel>(a.historyIn, (r0 + xi) * 8u);
        const TaaTexel h10 = right ? load_at<TaaTexel>(a.historyIn, (r0 + x1) * 8u) : zero;
        const TaaTexel h01 = below ? load_at<TaaTexel>(a.historyIn, (r1 + xi) * 8u) : zero;
        const TaaTexel h11 = right && below ? load_at<TaaTexel>(a.historyIn, (r1 + x1) * 8u) : zero;
        uint32_t hv[3];
        hv[0] = taa_bilinear(h00.rg & 0xFFFFu, h10.rg & 0xFFFFu, h01.rg & 0xFFFFu, h11.rg & 0xFFFFu, fx, fy);
        hv[1] = taa_bilinear(h00.rg >> 16, h10.rg >> 16, h01.rg >> 16, h11.rg >> 16, fx, fy);
        hv[2] = taa_bilinear(h00.ba & 0xFFFFu, h10.ba & 0xFFFFu, h01.ba & 0xFFFFu, h11.ba & 0xFFFFu, fx, fy);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // the clamp and step 6
            const uint32_t hc = (a.flags & kTaaNoClamp) ? hv[k] : taa_min(taa_max(hv[k], lo[k]), hi[k]);
            const uint32_t blended = (hc * (256u - weight) + c[k] * weight + 128u) >> 8;
            n[k] = hist ? blended : n[k];
        }
    }
    TaaTexel h;
    h.rg = n[0] | (n[1] << 16);
    h.ba = n[2] | (alpha << 24);
    __builtin_memcpy((char*)a.historyOut + (size_t)at * 8u, &h, 8);
    uint32_t o = alpha << 24;
#pragma unroll
    for (int k = 0; k < 3; ++k) o |= taa_min((n[k] + 128u) >> 8, 255u) << (8 * k);
    a.out[at] = o;
}

}  // namespace cry
