// ssr_core.hpp -- the body of crychic_ssr (include/crychic_hip.h states the definition), built for the device
// (ssr.hip) and for the host (tests/ssr_host).  One lane per pixel, an 8 x 8 pixel tile per wavefront (the fog pass's shape), so that
// neighbouring rays gather from neighbouring texels.  Per lane: the pixel's world point and its reflected ray are projected to a
// screen-space segment, the segment is marched in N steps against the depth plane, the first hit is refined by bisection, and the
// frame's texel at the hit is blended over the pixel's own with a Fresnel weight and two fades, in integers.
//
// The kernel's shape:
//   * a wavefront none of whose pixels reflects (sky, or roughness not below maxRoughness) copies 4 bytes a lane and has read the
//     frame, the depth plane and G1 only;
//   * steps go in batches of kSsrBatch: every sample address of a batch is computed and its depth load issued before the first
//     compare, so a batch costs one memory round trip.  A sample that ends its ray (outside the frame, past the far plane) loads
//     texel 0 (valid memory) and is resolved in order afterwards, so a later sample of the batch never counts;
//   * the march ends once no lane is still marching, the refinement and the composition run only if some lane has hit: all behind
//     votes, which only skip work whose result is already what it would be;
//   * no float is converted to an integer before the inside test has passed.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"
#include "light_core.hpp"
#include "fog_core.hpp"

namespace cry {

constexpr uint32_t kSsrMaxSteps = 64u;          // CRYCHIC_SSR_MAX_STEPS
constexpr uint32_t kSsrRefine = 4u;             // CRYCHIC_SSR_REFINE
// a wavefront covers an 8 x 8 pixel tile (lane = 8 y + x), a workgroup four tiles side by side: 32 x 8 pixels (fog_lane_x / fog_lane_y)
constexpr uint32_t kSsrTile = kFogTile, kSsrGroupW = kFogGroupW, kSsrThreads = kFogThreads;
constexpr uint32_t kSsrBatch = 8u;              // steps whose loads are in flight together

struct SsrParams { float maxDistance, thickness, bias, maxRoughness; uint32_t steps, edgeFade, intensity, reserved; };   // crychic_ssr_params

// the kernel's arguments (kernarg segment: every field is wave-uniform)
struct SsrArgs {
    const uint32_t* depth;
    const void* g0;
    const void* g1;
    const void* g2;
    const uint32_t* in;
    uint32_t* out;
    uint32_t W, H, row0, rowEnd, tilesX, N, E, intensity, h0, h1, h2;
    float ivp[16];          // InvViewProj
    float vp[16];           // ViewProj
    float eye[3];
    float A, B, sx, sy, hw, hh, Wf, Hf, invN, wmin, maxDistance, thickness, bias, maxRoughness;
};

struct SsrLaunch { SsrArgs args; uint32_t groups; };      // groups == 0: nothing to launch

// The launcher's plan and the host-side constants of the definition.  The matrices, eye and nearZ are the pass constants' fields.
// The caller has checked every argument (api.cpp).
inline SsrLaunch ssr_launch(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, float nearZ, const void* g0,
                            const void* g1, const void* g2, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H,
                            uint32_t row0, uint32_t rows, uint32_t formatFlags, const SsrParams& p)
{
    SsrLaunch L;
    SsrArgs& a = L.args;
    a.depth = depth; a.g0 = g0; a.g1 = g1; a.g2 = g2;
    a.in = reinterpret_cast<const uint32_t*>(in);
    a.out = reinterpret_cast<uint32_t*>(out);
    a.W = W; a.H = H; a.row0 = row0; a.rowEnd = row0 + rows; a.N = p.steps; a.E = p.edgeFade; a.intensity = p.intensity;
    a.tilesX = (W + kSsrGroupW - 1u) / kSsrGroupW;
    a.h0 = formatFlags & CRYCHIC_GBUFFER_G0_F16; a.h1 = formatFlags & CRYCHIC_GBUFFER_G1_F16; a.h2 = formatFlags & CRYCHIC_GBUFFER_G2_F16;
    for (int k = 0; k < 16; ++k) { a.ivp[k] = invViewProj[k]; a.vp[k] = viewProj[k]; }
    for (int k = 0; k < 3; ++k) a.eye[k] = eye[k];
    a.A = proj[10]; a.B = proj[11];
    a.sx = 2.0f / (float)W;
    a.sy = 2.0f / (float)H;
    a.Wf = (float)W; a.Hf = (float)H;
    a.hw = a.Wf * 0.5f; a.hh = a.Hf * 0.5f;
    a.invN = 1.0f / (float)p.steps;
    a.wmin = nearZ;
    a.maxDistance = p.maxDistance; a.thickness = p.thickness; a.bias = p.bias; a.maxRoughness = p.maxRoughness;
    const uint64_t groups = (uint64_t)a.tilesX * ((rows + kSsrTile - 1u) / kSsrTile);        // below 2^27: fits
    L.groups = (uint32_t)groups;
    return L;
}

// the screen-space segment of a ray: its start and the difference to its end, in pixels (x, y) and NDC depth (z)
struct SsrSegment { f3 s0, ds; };

// step 3: a homogeneous point to (pixels, pixels, NDC depth)
CRY_HD f3 ssr_screen(const SsrArgs& a, float hx, float hy, float hz, float hw)
{
    const float r = rcp(hw);
    return f3{ fma(hx * r, a.hw, a.hw), fma(-(hy * r), a.hh, a.hh), hz * r };
}

// One sample of the segment (steps 4 and 6): its ray depth and the texel index to load.  `ok`: inside the frame and in front of
// the far plane; otherwise the index is 0 and the sample ends its ray.
struct SsrSample { float dr; uint32_t idx; bool ok; };
CRY_HD SsrSample ssr_sample(const SsrArgs& a, const SsrSegment& g, float t)
{
    const float x = fma(g.ds.x, t, g.s0.x), y = fma(g.ds.y, t, g.s0.y);
    SsrSample s;
    s.dr = fma(g.ds.z, t, g.s0.z);
    s.ok = x >= 0.0f && x < a.Wf && y >= 0.0f && y < a.Hf && s.dr < 1.0f;
    // ok: x in [0, W), y in [0, H), both below 2^22: the index is below 2^28
    s.idx = s.ok ? mul24((uint32_t)y, a.W) + (uint32_t)x : 0u;
    return s;
}

// step 5: is the ray depth dr behind the depth word `word` by no less than bias and no more than thickness, in view units
CRY_HD bool ssr_hit(const SsrArgs& a, float dr, uint32_t word)
{
    const uint32_t w24 = word & 0x00FFFFFFu;
    const float ds = d24_to_float(w24);
    const float D = (dr - a.A) * (ds - a.A);
    const float num = a.B * (ds - dr);
    return w24 != 0x00FFFFFFu && dr > ds && a.bias * D <= num && num <= a.thickness * D;
}

// The hit colour of crychic_ssr, the end of step 6: a point sample of the frame.  A policy of ssr_pixel: called once by every lane that
// reaches step 7 (`hit`: the lane has a hit; otherwise hitIdx is 0 and the colour is not used), it returns the hit's texel, R, G and B
// in the low three bytes.  crychic_ssr_glossy's policy is in ssr_gloss_core.hpp.
struct SsrPointHit {
    template <class Any>
    CRY_HD uint32_t operator()(const SsrArgs& a, uint32_t, uint32_t, uint32_t hitIdx, float, bool, Any) const { return a.in[hitIdx]; }
};

// One pixel of the frame.  `any`: a vote over the lanes that run together (the device: the wavefront's active lanes; the host: the
// lane's own predicate).  It only skips work whose result would be what it already is; no result depends on it.  `colour`: the hit
// colour's policy.
template <class Any, class HitColour>
CRY_HD void ssr_pixel(const SsrArgs& a, uint32_t px, uint32_t py, Any any, const HitColour& colour)
{
    const uint32_t at = py * a.W + px;                         // below 2^28
    const uint32_t texel = a.in[at];
    // step 1
    const uint32_t word = a.depth[at] & 0x00FFFFFFu;
    const f4a G1 = gbuffer_load(a.g1, at, a.h1);
    const float rough = G1.w;
    const bool reflects = word != 0x00FFFFFFu && rough < a.maxRoughness;
    if (!any(reflects)) { a.out[at] = texel; return; }
    // step 2: the world point (crychic_fog's steps 2 and 3) and the reflected ray
    const f4a G2 = gbuffer_load(a.g2, at, a.h2);
    const float d = d24_to_float(word);
    const float nx = fma((float)px + 0.5f, a.sx, -1.0f);
    const float ny = fma((float)py + 0.5f, -a.sy, 1.0f);
    const float wx = mulcol(nx, ny, d, 1.0f, a.ivp), wy = mulcol(nx, ny, d, 1.0f, a.ivp + 4), wz = mulcol(nx, ny, d, 1.0f, a.ivp + 8);
    const float rw = rcp(mulcol(nx, ny, d, 1.0f, a.ivp + 12));
    const f3 P{ wx * rw, wy * rw, wz * rw };
    const f3 V = normalize3(f3{ P.x - a.eye[0], P.y - a.eye[1], P.z - a.eye[2] });
    const f3 Nw = normalize3(f3{ G2.x, G2.y, G2.z });
    const f3 R = reflect3(V, Nw);
    // step 3
    const float h0x = mulcol(P.x, P.y, P.z, 1.0f, a.vp), h0y = mulcol(P.x, P.y, P.z, 1.0f, a.vp + 4), h0z = mulcol(P.x, P.y, P.z, 1.0f, a.vp + 8),
                h0w = mulcol(P.x, P.y, P.z, 1.0f, a.vp + 12);
    f3 Q{ fma(R.x, a.maxDistance, P.x), fma(R.y, a.maxDistance, P.y), fma(R.z, a.maxDistance, P.z) };
    float h1w = mulcol(Q.x, Q.y, Q.z, 1.0f, a.vp + 12);
    if (h1w < a.wmin) {         // the end is behind the near plane: shorten the ray to it
        const float tt = (h0w - a.wmin) * rcp(h0w - h1w);
        const float md = a.maxDistance * tt;
        Q = f3{ fma(R.x, md, P.x), fma(R.y, md, P.y), fma(R.z, md, P.z) };
        h1w = mulcol(Q.x, Q.y, Q.z, 1.0f, a.vp + 12);
    }
    const float h1x = mulcol(Q.x, Q.y, Q.z, 1.0f, a.vp), h1y = mulcol(Q.x, Q.y, Q.z, 1.0f, a.vp + 4), h1z = mulcol(Q.x, Q.y, Q.z, 1.0f, a.vp + 8);
    bool live = reflects && h0w > a.wmin;                      // still marching
    SsrSegment g;
    g.s0 = ssr_screen(a, h0x, h0y, h0z, h0w);
    const f3 s1 = ssr_screen(a, h1x, h1y, h1z, h1w);
    g.ds = f3{ s1.x - g.s0.x, s1.y - g.s0.y, s1.z - g.s0.z };
    // steps 4 and 5
    const float jit = fog_jitter(px, py);
    bool hit = false;
    float tHit = 0.0f, tLo = 0.0f;
    uint32_t hitIdx = 0u;
    for (uint32_t i0 = 0; i0 < a.N && any(live); i0 += kSsrBatch) {
        SsrSample s[kSsrBatch];
        uint32_t tex[kSsrBatch];
#pragma unroll
        for (uint32_t k = 0; k < kSsrBatch; ++k) {
            s[k] = ssr_sample(a, g, ((float)(i0 + k) + jit) * a.invN);
            tex[k] = load_at<uint32_t>(a.depth, s[k].idx * 4u);
        }
#pragma unroll
        for (uint32_t k = 0; k < kSsrBatch; ++k) {
            const bool run = live && i0 + k < a.N;
            const bool h = run && s[k].ok && s[k].idx != at && ssr_hit(a, s[k].dr, tex[k]);
            if (h) {
                hit = true;
                hitIdx = s[k].idx;
                tHit = ((float)(i0 + k) + jit) * a.invN;
                tLo = (i0 + k == 0u) ? 0.0f : ((float)(i0 + k - 1u) + jit) * a.invN;
            }
            live = live && !h && !(run && !s[k].ok);
        }
    }
    if (!any(hit)) { a.out[at] = texel; return; }
    // step 6
    float tHi = tHit;
#pragma unroll
    for (uint32_t r = 0; r < kSsrRefine; ++r) {
        const float tm = (tLo + tHi) * 0.5f;
        const SsrSample m = ssr_sample(a, g, tm);
        const uint32_t w = load_at<uint32_t>(a.depth, m.idx * 4u);
        const bool pass = hit && m.ok && m.idx != at && ssr_hit(a, m.dr, w);
        tHi = pass ? tm : tHi;
        tLo = pass ? tLo : tm;
        hitIdx = pass ? m.idx : hitIdx;
    }
    tHit = tHi;
    // steps 7 to 9: integers from here on
    const f4a G0 = gbuffer_load(a.g0, at, a.h0);
    const uint32_t src = colour(a, px, py, hitIdx, rough, hit, any);
    const float f0 = 1.0f - saturate(dot3(Nw, R));
    const float f2 = f0 * f0;
    const float f5 = (f2 * f2) * f0;
    const uint32_t hy = hitIdx / a.W, hx = hitIdx - hy * a.W;
    const uint32_t ex = hx < a.W - 1u - hx ? hx : a.W - 1u - hx, ey = hy < a.H - 1u - hy ? hy : a.H - 1u - hy;
    const uint32_t e = ex < ey ? ex : ey;
    const uint32_t fe = ((e < a.E ? e : a.E) << 16) / a.E;
    const uint32_t tq = hit ? (uint32_t)(tHit * 65536.0f) : 0u;        // a hit's t lies in [0, 1)
    const uint32_t fd4 = 4u * (65536u - tq);
    const uint32_t fd = fd4 < 65536u ? fd4 : 65536u;
    const float alb[3] = { G1.x, G1.y, G1.z };
    uint32_t o = texel & 0xFF000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float R0 = lerpf(0.04f, alb[c], G0.w);
        const float wgt = (1.0f - rough) * fma(1.0f - R0, f5, R0);
        const uint32_t wq = (uint32_t)fma(clampf(wgt, 0.0f, 1.0f), 65536.0f, 0.5f);     // 0 .. 65536
        const uint32_t k1 = (uint32_t)(((uint64_t)wq * fe) >> 16);
        const uint32_t k2 = (uint32_t)(((uint64_t)k1 * fd) >> 16);
        const uint32_t K = (k2 * a.intensity) >> 8;                                      // 0 .. 65536
        const uint32_t own = (texel >> (8 * c)) & 255u, far = (src >> (8 * c)) & 255u;
        o |= ((own * (65536u - K) + far * K + 32768u) >> 16) << (8 * c);
    }
    a.out[at] = hit ? o : texel;
}

template <class Any>
CRY_HD void ssr_pixel(const SsrArgs& a, uint32_t px, uint32_t py, Any any) { ssr_pixel(a, px, py, any, SsrPointHit{}); }

}  // namespace cry
