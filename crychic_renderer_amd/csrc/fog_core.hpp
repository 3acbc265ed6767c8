// fog_core.hpp -- the body of crychic_fog (include/crychic_hip.h states the definition), built for the device
// (fog.hip) and for the host (tests/fog_host).  One lane per pixel, an 8 x 8 pixel tile per wavefront: the pixel's view ray is reconstructed from its depth, marched in
// N steps through the cascade maps with one point compare per step, and the frame's texel is composed with the transmittance, the
// ambient and the sun in-scatter in integers.
//
// The march, per lane:
//   * the shadow coordinates of a sample are s = a[j] + f b[j] with b[j] the ray through cascade j's transform: the four b[j] are
//     computed once in front of the march (36 fmas), a[j] on the host;
//   * t rises with the step, so the cascade index only ever goes up: the lane keeps its current cascade's a, b, map pointer and
//     upper limit in registers and re-selects them only at a step whose t is not below that limit.  The re-selection is a function
//     of t alone, so running it for a lane that does not need it changes nothing: the device skips it behind a wave vote, the host
//     build behind the lane's own predicate;
//   * steps go in batches of kFogBatch: every texel address of a batch is computed and its load issued before the first compare, so a
//     batch costs one memory round trip, not kFogBatch.  A sample outside its map, or beyond the last cascade, loads texel 0 of its
//     map (valid memory) and carries s.z = -1, which every decoded depth (>= 0) passes: lit, as the definition says.
// qi == 65536 in every lane of a wave is a copy (T stays 65536 and S stays 0: step 9 gives in back), also behind a vote.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kFogMaxSteps = 64u;          // CRYCHIC_FOG_MAX_STEPS
// a wavefront covers an 8 x 8 pixel tile (lane = 8 y + x), a workgroup four tiles side by side: 32 x 8 pixels
constexpr uint32_t kFogTile = 8u, kFogWaves = 4u, kFogGroupW = kFogTile * kFogWaves, kFogThreads = 64u * kFogWaves;
CRY_HD uint32_t fog_lane_x(uint32_t thread) { return (thread >> 6) * kFogTile + (thread & (kFogTile - 1u)); }     // within the workgroup
CRY_HD uint32_t fog_lane_y(uint32_t thread) { return (thread >> 3) & (kFogTile - 1u); }
constexpr uint32_t kFogBatch = 8u;              // steps whose loads are in flight together

struct FogParams { float density, maxDistance; uint32_t steps; uint8_t ambient[4], sun[4]; uint32_t reserved[3]; };   // crychic_fog_params

// the kernel's arguments (kernarg segment: every field is wave-uniform)
struct FogArgs {
    const uint32_t* depth;
    const uint32_t* map[4];
    const uint32_t* in;
    uint32_t* out;
    uint32_t W, row0, rowEnd, tilesX, dim, N;
    float ivp[16];          // InvViewProj
    float eye[3];
    float m[4][3][3];       // ShadowTransforms[j] + 4c, floats 0 .. 2
    float a[4][3];          // mulcol1(Eye, ShadowTransforms[j] + 4c)
    float c, invN, sx, sy, dimf, maxDistance;
    uint32_t ambient[3], sun[3];
};

struct FogLaunch { FogArgs args; uint32_t groups; };      // groups == 0: nothing to launch

// The launcher's plan and the host-side constants of the definition.  invViewProj, eye, shadowTransforms: the pass constants' fields.
// The caller has checked every argument (api.cpp).
inline FogLaunch fog_launch(const float* invViewProj, const float* eye, const float (*shadowTransforms)[16], const uint32_t* depth,
                            const uint32_t* const* maps, uint32_t dim, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                            uint32_t rows, const FogParams& p)
{
    FogLaunch L;
    FogArgs& a = L.args;
    a.depth = depth;
    for (int j = 0; j < 4; ++j) a.map[j] = maps[j];
    a.in = reinterpret_cast<const uint32_t*>(in);
    a.out = reinterpret_cast<uint32_t*>(out);
    a.W = W; a.row0 = row0; a.rowEnd = row0 + rows; a.dim = dim; a.N = p.steps;
    a.tilesX = (W + kFogGroupW - 1u) / kFogGroupW;
    for (int k = 0; k < 16; ++k) a.ivp[k] = invViewProj[k];
    for (int k = 0; k < 3; ++k) { a.eye[k] = eye[k]; a.ambient[k] = p.ambient[k]; a.sun[k] = p.sun[k]; }
    for (int j = 0; j < 4; ++j)
        for (int c = 0; c < 3; ++c) {
            const float* col = shadowTransforms[j] + 4 * c;
            for (int k = 0; k < 3; ++k) a.m[j][c][k] = col[k];
            a.a[j][c] = mulcol1(eye[0], eye[1], eye[2], col);
        }
    a.invN = 1.0f / (float)p.steps;
    a.c = -(p.density * 1.44269504f) * a.invN;
    a.sx = 2.0f / (float)W;
    a.sy = 2.0f / (float)H;
    a.dimf = (float)dim;
    a.maxDistance = p.maxDistance;
    const uint64_t groups = (uint64_t)a.tilesX * ((rows + kFogTile - 1u) / kFogTile);      // below 2^27: fits
    L.groups = (uint32_t)groups;
    return L;
}

// (B[py & 3][px & 3] + 0.5) / 16 of the 4 x 4 Bayer matrix { 0, 8, 2, 10; 12, 4, 14, 6; 3, 11, 1, 9; 15, 7, 13, 5 }: sixteen nibbles,
// rows 0 and 1 in one word and rows 2 and 3 in the other, lowest nibble first
CRY_HD float fog_jitter(uint32_t px, uint32_t py)
{
    const uint32_t word = (py & 2u) ? 0x5D7F91B3u : 0x6E4CA280u;
    const uint32_t b = (word >> ((((py & 1u) << 2) + (px & 3u)) << 2)) & 15u;
    return ((float)b + 0.5f) * 0.0625f;
}

// the lane's current cascade: what step 8 needs of it
struct FogCascade {
    float bx, by, bz, ax, ay, az;
    const uint32_t* map;
    float limit;            // the cascade ends where t is no longer below this
    bool beyond;            // t is not below 100: the sample is lit
};

// the value of the first true condition's slot, v3 if none: on values, not lvalues, so that it stays a chain of selects between
// registers and never becomes a load through a selected address
template <class T>
CRY_HD T fog_sel(bool c0, bool c1, bool c2, T v0, T v1, T v2, T v3) { return c0 ? v0 : (c1 ? v1 : (c2 ? v2 : v3)); }

CRY_HD FogCascade fog_select(const FogArgs& a, const float (&b)[4][3], float t)
{
    const bool c0 = t < 30.0f, c1 = t < 50.0f, c2 = t < 80.0f, c3 = t < 100.0f;
    FogCascade s;
    s.bx = fog_sel(c0, c1, c2, b[0][0], b[1][0], b[2][0], b[3][0]);
    s.by = fog_sel(c0, c1, c2, b[0][1], b[1][1], b[2][1], b[3][1]);
    s.bz = fog_sel(c0, c1, c2, b[0][2], b[1][2], b[2][2], b[3][2]);
    s.ax = fog_sel(c0, c1, c2, a.a[0][0], a.a[1][0], a.a[2][0], a.a[3][0]);
    s.ay = fog_sel(c0, c1, c2, a.a[0][1], a.a[1][1], a.a[2][1], a.a[3][1]);
    s.az = fog_sel(c0, c1, c2, a.a[0][2], a.a[1][2], a.a[2][2], a.a[3][2]);
    s.map = fog_sel(c0, c1, c2, a.map[0], a.map[1], a.map[2], a.map[3]);
    s.limit = fog_sel(c0, c1, c2, 30.0f, 50.0f, 80.0f, c3 ? 100.0f : __builtin_inff());
    s.beyond = !c3;
    return s;
}

// One pixel of the frame.  `any`: a vote over the lanes that run together (the device: the wavefront's active lanes; the host: the
// lane's own predicate).  It only skips work whose result would be what it already is; no result depends on it.
template <class Any>
CRY_HD void fog_pixel(const FogArgs& a, uint32_t px, uint32_t py, Any any)
{
    const uint32_t at = py * a.W + px;                         // below 2^28
    const uint32_t texel = a.in[at];
    // steps 1 .. 5: the ray and its transmittance per step
    const float d = d24_to_float(a.depth[at]);
    const float nx = fma((float)px + 0.5f, a.sx, -1.0f);
    const float ny = fma((float)py + 0.5f, -a.sy, 1.0f);
    const float hx = mulcol(nx, ny, d, 1.0f, a.ivp), hy = mulcol(nx, ny, d, 1.0f, a.ivp + 4), hz = mulcol(nx, ny, d, 1.0f, a.ivp + 8);
    const float rw = rcp(mulcol(nx, ny, d, 1.0f, a.ivp + 12));
    const f3 r{ hx * rw - a.eye[0], hy * rw - a.eye[1], hz * rw - a.eye[2] };
    const float L = len_from_sq(dot3(r, r));
    const float Lc = __builtin_fminf(L, a.maxDistance);
    const float invL = rcp(L);
    const float q = det_exp2(a.c * Lc);
    const uint32_t qi = (uint32_t)fma(q, 65536.0f, 0.5f);      // q in [2^-125, 1]: 0 .. 65536
    if (!any(qi != 65536u)) { a.out[at] = texel; return; }     // exact: every T is 65536 and S is 0
    // step 6
    const float stepLen = Lc * a.invN;
    const float jit = fog_jitter(px, py);
    float b[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[j][c] = fma(r.z, a.m[j][c][2], fma(r.y, a.m[j][c][1], r.x * a.m[j][c][0]));
    // steps 7 and 8
    uint32_t T = 65536u, S = 0u;
    FogCascade cs = fog_select(a, b, jit * stepLen);           // ((float)0 + jit) * stepLen
    for (uint32_t i0 = 0; i0 < a.N; i0 += kFogBatch) {
        float sz[kFogBatch];
        uint32_t tex[kFogBatch];
#pragma unroll
        for (uint32_t k = 0; k < kFogBatch; ++k) {
            sz[k] = -1.0f;
            tex[k] = 0u;
            if (i0 + k < a.N) {
                const float t = ((float)(i0 + k) + jit) * stepLen;
                if (any(!(t < cs.limit))) cs = fog_select(a, b, t);
                const float f = t * invL;
                const float fx = fma(cs.bx, f, cs.ax) * a.dimf, fy = fma(cs.by, f, cs.ay) * a.dimf;
                const bool inside = !cs.beyond && fx >= 0.0f && fx < a.dimf && fy >= 0.0f && fy < a.dimf;
                // inside: fx, fy in [0, dim), dim <= 16384: the index is below 2^28
                const uint32_t idx = inside ? mul24((uint32_t)fy, a.dim) + (uint32_t)fx : 0u;
                sz[k] = inside ? fma(cs.bz, f, cs.az) : -1.0f;
                tex[k] = load_at<uint32_t>(cs.map, idx * 4u);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kFogBatch; ++k)
            if (i0 + k < a.N) {
                const uint32_t Tn = (uint32_t)(((uint64_t)T * qi + 32768u) >> 16);
                S += (sz[k] <= d24_to_float(tex[k])) ? T - Tn : 0u;
                T = Tn;
            }
    }
    // step 9
    const uint32_t U = 65536u - T;
    uint32_t o = texel & 0xFF000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t v = (((texel >> (8 * c)) & 255u) * T + a.ambient[c] * U + a.sun[c] * S + 32768u) >> 16;
        o |= (v < 255u ? v : 255u) << (8 * c);
    }
    a.out[at] = o;
}

}  // namespace cry
