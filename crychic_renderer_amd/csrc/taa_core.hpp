// taa_core.hpp -- the body of crychic_taa (include/crychic_hip.h states the definition), built for the device
// (taa.hip) and for the host (tests/taa_host).  One lane per pixel, an 8 x 8 pixel tile per wavefront, four tiles side by side per
// workgroup, as in the fog pass.  Lanes share nothing: a lane reads the 3 x 3 texels of `in` around its pixel straight from memory
// (the tile's rows are 32 bytes apart in a wave and 128 bytes in a workgroup, so the nine loads of a wave fall into the cache lines
// its neighbours fetch anyway; no LDS, no barrier), reconstructs its world point from the depth plane, projects it through the two
// view-projections and gathers its history with 8-byte loads.
//
// Two kinds of wave vote, and each only skips work whose result is already known:
//   * no lane of the wave has history (a RESET frame, or a tile whose history lies outside the previous frame): nothing is gathered;
//   * a tap whose weight is 0 contributes 0 exactly: fx == 0 in every lane drops the two right-hand taps, fy == 0 the two lower
//     ones (a still camera reads one history texel per pixel, not four).  A dropped tap is taken as 0, which its weight of 0 makes
//     of it anyway.
// A lane without history in a wave that gathers reads texel 0 of the plane (valid memory) and discards it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kTaaReset = 1u, kTaaNoClamp = 2u;        // CRYCHIC_TAA_RESET, CRYCHIC_TAA_NO_CLAMP
constexpr uint32_t kTaaMaxSide = 1u << 22;                   // W, H: the history position in 1/256 texel stays below 2^30
// a wavefront covers an 8 x 8 pixel tile (lane = 8 y + x), a workgroup four tiles side by side: 32 x 8 pixels
constexpr uint32_t kTaaTile = 8u, kTaaWaves = 4u, kTaaGroupW = kTaaTile * kTaaWaves, kTaaThreads = 64u * kTaaWaves;
CRY_HD uint32_t taa_lane_x(uint32_t thread) { return (thread >> 6) * kTaaTile + (thread & (kTaaTile - 1u)); }     // within the workgroup
CRY_HD uint32_t taa_lane_y(uint32_t thread) { return (thread >> 3) & (kTaaTile - 1u); }

struct TaaParams { uint32_t blend, flags, reserved[6]; };   // crychic_taa_params

// the kernel's arguments (kernarg segment: every field is wave-uniform)
struct TaaArgs {
    const uint32_t* depth;
    const uint32_t* in;
    const void* historyIn;      // four uint16_t per texel; NULL only with kTaaReset
    void* historyOut;
    uint32_t* out;
    uint32_t W, H, row0, rowEnd, tilesX, blend, flags;
    float ivp[16];              // InvViewProj of the frame's own constants
    float cur[3][4], prev[3][4];        // columns 0, 1 and 3 of the unjittered view-projections
    float sx, sy, hw, hh, xmax, ymax;
};

struct TaaLaunch { TaaArgs args; uint32_t groups; };      // groups == 0: nothing to launch

// The launcher's plan and the host-side constants of the definition.  The caller has checked every argument (api.cpp).
inline TaaLaunch taa_launch(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, const uint8_t* in,
                            const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                            const TaaParams& p)
{
    TaaLaunch L;
    TaaArgs& a = L.args;
    a.depth = depth;
    a.in = reinterpret_cast<const uint32_t*>(in);
    a.historyIn = historyIn;
    a.historyOut = historyOut;
    a.out = reinterpret_cast<uint32_t*>(out);
    a.W = W; a.H = H; a.row0 = row0; a.rowEnd = row0 + rows; a.blend = p.blend; a.flags = p.flags;
    a.tilesX = (W + kTaaGroupW - 1u) / kTaaGroupW;
    for (int k = 0; k < 16; ++k) a.ivp[k] = invViewProj[k];
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 4; ++k) {
            a.cur[c][k] = curViewProj[4 * (c == 2 ? 3 : c) + k];
            a.prev[c][k] = prevViewProj[4 * (c == 2 ? 3 : c) + k];
        }
    a.sx = 2.0f / (float)W;
    a.sy = 2.0f / (float)H;
    a.hw = 0.5f * (float)W;
    a.hh = 0.5f * (float)H;
    a.xmax = (float)((W - 1u) * 256u);
    a.ymax = (float)((H - 1u) * 256u);
    const uint64_t groups = (uint64_t)a.tilesX * ((rows + kTaaTile - 1u) / kTaaTile);      // below 2^27: fits
    L.groups = (uint32_t)groups;
    return L;
}

struct TaaTexel { uint32_t rg, ba; };           // a history texel: R | G << 16, B | A << 16

CRY_HD uint32_t taa_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
CRY_HD uint32_t taa_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// step 4's filter of one channel
CRY_HD uint32_t taa_bilinear(uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11, uint32_t fx, uint32_t fy)
{
    const uint32_t top = t00 * (256u - fx) + t10 * fx, bot = t01 * (256u - fx) + t11 * fx;
    return (top * (256u - fy) + bot * fy + 32768u) >> 16;
}

// One pixel of the frame.  `any`: a vote over the lanes that run together (the device: the wavefront's active lanes; the host: the
// lane's own predicate).  It only skips work whose result would be what it already is; no result depends on it.
template <class Any>
CRY_HD void taa_pixel(const TaaArgs& a, uint32_t px, uint32_t py, Any any)
{
    const uint32_t at = py * a.W + px;                         // below 2^28
    // step 1: the neighbourhood, clamped to the frame
    const uint32_t xl = px ? px - 1u : 0u, xr = px + 1u < a.W ? px + 1u : px;
    const uint32_t rowU = (py ? py - 1u : 0u) * a.W, rowC = py * a.W, rowD = (py + 1u < a.H ? py + 1u : py) * a.W;
    const uint32_t nb[9] = { a.in[rowU + xl], a.in[rowU + px], a.in[rowU + xr], a.in[rowC + xl], a.in[rowC + px], a.in[rowC + xr],
                             a.in[rowD + xl], a.in[rowD + px], a.in[rowD + xr] };
    const uint32_t texel = nb[4];
    const uint32_t rawDepth = a.depth[at];
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
        c[k] = (texel >> (8 * k)) & 255u;
    }
    const uint32_t alpha = texel >> 24;
    // steps 2 and 3: the world point and its velocity in pixels
    bool hist = false;
    float fxp = 0.0f, fyp = 0.0f;
    if (!(a.flags & kTaaReset)) {                               // wave-uniform
        const float d = d24_to_float(rawDepth);
        const float nx = fma((float)px + 0.5f, a.sx, -1.0f);
        const float ny = fma((float)py + 0.5f, -a.sy, 1.0f);
        const float hx = mulcol(nx, ny, d, 1.0f, a.ivp), hy = mulcol(nx, ny, d, 1.0f, a.ivp + 4), hz = mulcol(nx, ny, d, 1.0f, a.ivp + 8);
        const float rw = rcp(mulcol(nx, ny, d, 1.0f, a.ivp + 12));
        const float Px = hx * rw, Py = hy * rw, Pz = hz * rw;
        const float a0 = mulcol1(Px, Py, Pz, a.cur[0]), a1 = mulcol1(Px, Py, Pz, a.cur[1]), a3 = mulcol1(Px, Py, Pz, a.cur[2]);
        const float b0 = mulcol1(Px, Py, Pz, a.prev[0]), b1 = mulcol1(Px, Py, Pz, a.prev[1]), b3 = mulcol1(Px, Py, Pz, a.prev[2]);
        const float ra = rcp(a3), rb = rcp(b3);
        const float vx = (a0 * ra - b0 * rb) * a.hw;
        const float vy = (b1 * rb - a1 * ra) * a.hh;
        // step 4
        fxp = ((float)px - vx) * 256.0f;
        fyp = ((float)py - vy) * 256.0f;
        hist = b3 > 0.0f && fxp >= 0.0f && fxp <= a.xmax && fyp >= 0.0f && fyp <= a.ymax;
    }
    uint32_t n[3] = { c[0] << 8, c[1] << 8, c[2] << 8 };
    if (any(hist)) {
        // in range with history: below 2^30.  Without: texel 0, never used
        const uint32_t X = hist ? (uint32_t)(int)__builtin_floorf(fxp) : 0u, Y = hist ? (uint32_t)(int)__builtin_floorf(fyp) : 0u;
        const uint32_t xi = X >> 8, fx = X & 255u, yi = Y >> 8, fy = Y & 255u;
        const uint32_t x1 = xi + 1u < a.W ? xi + 1u : xi, y1 = yi + 1u < a.H ? yi + 1u : yi;
        const uint32_t r0 = mul24(yi, a.W), r1 = mul24(y1, a.W);           // rows below 2^22, texel indices below 2^28: byte offsets below 2^31
        const bool right = any(hist && fx != 0u), below = any(hist && fy != 0u);
        const TaaTexel zero = { 0u, 0u };
        const TaaTexel t00 = load_at<TaaTexel>(a.historyIn, (r0 + xi) * 8u);
        const TaaTexel t10 = right ? load_at<TaaTexel>(a.historyIn, (r0 + x1) * 8u) : zero;
        const TaaTexel t01 = below ? load_at<TaaTexel>(a.historyIn, (r1 + xi) * 8u) : zero;
        const TaaTexel t11 = right && below ? load_at<TaaTexel>(a.historyIn, (r1 + x1) * 8u) : zero;
        uint32_t hv[3];
        hv[0] = taa_bilinear(t00.rg & 0xFFFFu, t10.rg & 0xFFFFu, t01.rg & 0xFFFFu, t11.rg & 0xFFFFu, fx, fy);
        hv[1] = taa_bilinear(t00.rg >> 16, t10.rg >> 16, t01.rg >> 16, t11.rg >> 16, fx, fy);
        hv[2] = taa_bilinear(t00.ba & 0xFFFFu, t10.ba & 0xFFFFu, t01.ba & 0xFFFFu, t11.ba & 0xFFFFu, fx, fy);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // steps 5 and 6
            const uint32_t hc = (a.flags & kTaaNoClamp) ? hv[k] : taa_min(taa_max(hv[k], lo[k]), hi[k]);
            const uint32_t blended = (hc * (256u - a.blend) + (c[k] << 8) * a.blend + 128u) >> 8;
            n[k] = hist ? blended : n[k];
        }
    }
    // step 7
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
