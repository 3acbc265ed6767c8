// motion_blur_core.hpp -- the bodies of crychic_motion_blur (include/crychic_hip.h states the definition), built
// for the device (motion_blur.hip) and for the host (tests/motion_blur_host).  Two launches, both with one 256-thread workgroup per
// 16 x 16 pixel tile (thread = 16 y + x: a wavefront covers four rows of the tile):
//   * velocity: a lane reprojects its pixel as taa_core.hpp does (the same operations in the same order, restated here so that
//     taa.hip's machine code stays what it is), writes its 8-byte workspace texel and enters the tile's reduction with the key
//     len << 32 | word.  How the 256 keys are reduced is the caller's (`Reduce`): the device exchanges lanes inside a wavefront and
//     passes four keys through LDS, the host takes the maximum over its walk.  Equal keys are equal words, so the order is free.
//   * gather: the workgroup reads the nine tile words around its tile itself (wave-uniform addresses), so the dominant velocity vN
//     is wave-uniform: a still neighbourhood is a uniform branch that stores the texels the threads already hold, and in the sample loop
//     the offsets are the same in every lane, so a wavefront's gathers are its own footprint shifted: rows of 128 and 64 contiguous bytes.
// The sample loop issues kMbBatch samples' loads (one 8-byte workspace texel and one 4-byte colour each) before the first use.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"

namespace cry {

constexpr uint32_t kMbMaxSide = 1u << 22;                   // W, H: as the temporal anti-aliasing
constexpr uint32_t kMbTile = 16u, kMbThreads = kMbTile * kMbTile;
constexpr uint32_t kMbStill = 8u;                          // len(vN) below this, half a pixel: the pixel is copied
constexpr uint32_t kMbBatch = 4u;                          // samples whose loads are in flight together

struct MotionBlurParams { uint32_t shutter, samples, maxRadius, flags, reserved[4]; };   // crychic_motion_blur_params

CRY_HD uint32_t mb_tiles(uint32_t n) { return (n + kMbTile - 1u) / kMbTile; }
inline size_t mb_tile_offset(uint32_t W, uint32_t H) { return (size_t)W * H * 8u; }
inline size_t mb_workspace_bytes(uint32_t W, uint32_t H) { return mb_tile_offset(W, H) + (size_t)mb_tiles(W) * mb_tiles(H) * 4u; }

// the arguments of the velocity kernel (kernarg segment: every field is wave-uniform)
struct MbVelocityArgs {
    const uint32_t* depth;
    void* velocity;             // W x H texels of 8 bytes
    uint32_t* tiles;            // tilesX x tilesY words
    uint32_t W, H, tilesX;
    int32_t qmax;               // 16 R
    float ivp[16];              // InvViewProj of the frame's constants
    float cur[3][4], prev[3][4];        // columns 0, 1 and 3 of the unjittered view-projections
    float sx, sy, hw, hh, shutter, radius;
};

struct MbGatherArgs {
    const uint32_t* in;
    uint32_t* out;
    const void* velocity;
    const uint32_t* tiles;
    uint32_t W, H, row0, rowEnd, tilesX, tilesY, tileRow0;
    uint32_t samples, shift;    // N and log2(16 N)
};

struct MbVelocityLaunch { MbVelocityArgs args; uint32_t groups; };
struct MbGatherLaunch { MbGatherArgs args; uint32_t groups; };       // groups == 0: nothing to launch

// The launchers' plans and the host-side constants of the definition.  The caller has checked every argument (api.cpp).
inline MbVelocityLaunch mb_velocity_launch(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth,
                                           uint32_t W, uint32_t H, const MotionBlurParams& p, void* workspace)
{
    MbVelocityLaunch L;
    MbVelocityArgs& a = L.args;
    a.depth = depth;
    a.velocity = workspace;
    a.tiles = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + mb_tile_offset(W, H));
    a.W = W; a.H = H; a.tilesX = mb_tiles(W);
    a.qmax = (int32_t)(16u * p.maxRadius);
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
    a.shutter = (float)p.shutter * 0.00390625f;             // a multiple of 1/256 up to 1: exact
    a.radius = (float)p.maxRadius;
    L.groups = a.tilesX * mb_tiles(H);                      // below 2^20: at most 2^28 pixels
    return L;
}

inline MbGatherLaunch mb_gather_launch(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const MotionBlurParams& p,
                                       const void* workspace)
{
    MbGatherLaunch L;
    MbGatherArgs& a = L.args;
    a.in = reinterpret_cast<const uint32_t*>(in);
    a.out = reinterpret_cast<uint32_t*>(out);
    a.velocity = workspace;
    a.tiles = reinterpret_cast<const uint32_t*>(static_cast<const char*>(workspace) + mb_tile_offset(W, H));
    a.W = W; a.H = H; a.row0 = row0; a.rowEnd = row0 + rows;
    a.tilesX = mb_tiles(W); a.tilesY = mb_tiles(H);
    a.tileRow0 = row0 / kMbTile;
    a.samples = p.samples;
    a.shift = 4u;
    for (uint32_t n = p.samples; n > 1u; n >>= 1) ++a.shift;
    L.groups = rows ? a.tilesX * ((row0 + rows - 1u) / kMbTile - a.tileRow0 + 1u) : 0u;
    return L;
}

struct MbTexel { uint32_t word, depth; };       // a workspace texel: (uint16)qx | (uint16)qy << 16, depth & 0xFFFFFF

CRY_HD int32_t mb_abs(int32_t v) { return v < 0 ? -v : v; }
CRY_HD int32_t mb_max(int32_t a, int32_t b) { return a > b ? a : b; }
CRY_HD int32_t mb_qx(uint32_t word) { return (int32_t)(int16_t)(word & 0xFFFFu); }
CRY_HD int32_t mb_qy(uint32_t word) { return (int32_t)(int16_t)(word >> 16); }
CRY_HD uint32_t mb_len(uint32_t word) { return (uint32_t)mb_max(mb_abs(mb_qx(word)), mb_abs(mb_qy(word))); }
CRY_HD uint64_t mb_key(uint32_t word) { return ((uint64_t)mb_len(word) << 32) | word; }

// step A.4
CRY_HD int32_t mb_quantise(float s, int32_t qmax)
{
    const int32_t q = (int32_t)__builtin_floorf(fma(s, 16.0f, 0.5f));      // |s| is at most R (1 + 2^-22): far inside int
    return q < -qmax ? -qmax : (q > qmax ? qmax : q);
}

// Step A for one pixel of the frame: its workspace texel.
CRY_HD MbTexel mb_velocity_texel(const MbVelocityArgs& a, uint32_t px, uint32_t py)
{
    const uint32_t rawDepth = a.depth[py * a.W + px];
    // TAA's steps 2 and 3
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
    // finite: the magnitude is below infinity (false for NaN)
    const bool valid = a3 > 0.0f && b3 > 0.0f && __builtin_fabsf(vx) < __builtin_inff() && __builtin_fabsf(vy) < __builtin_inff();
    // steps 2 .. 4
    float sx = (valid ? vx : 0.0f) * a.shutter, sy = (valid ? vy : 0.0f) * a.shutter;
    const float m = __builtin_fmaxf(__builtin_fabsf(sx), __builtin_fabsf(sy));
    if (m > a.radius) {
        const float k = a.radius * rcp(m);
        sx *= k;
        sy *= k;
    }
    const int32_t qx = mb_quantise(sx, a.qmax), qy = mb_quantise(sy, a.qmax);
    MbTexel t;
    t.word = ((uint32_t)qx & 0xFFFFu) | ((uint32_t)qy << 16);
    t.depth = rawDepth & 0x00FFFFFFu;
    return t;
}

// One thread of the velocity workgroup of tile (tx, ty).  Every thread of the workgroup calls it (the reduction meets a barrier on
// the device): a thread outside the frame enters the reduction with key 0, which no key of a pixel is below.  reduce(key, thread)
// returns the tile's largest key to the thread(s) for which it returns true in `owner`.
template <class Reduce>
CRY_HD void mb_velocity_thread(const MbVelocityArgs& a, uint32_t tx, uint32_t ty, uint32_t thread, Reduce reduce)
{
    const uint32_t px = tx * kMbTile + (thread & (kMbTile - 1u)), py = ty * kMbTile + (thread >> 4);
    uint64_t key = 0u;
    if (px < a.W && py < a.H) {
        const MbTexel t = mb_velocity_texel(a, px, py);
        __builtin_memcpy((char*)a.velocity + (size_t)(py * a.W + px) * 8u, &t, 8);         // below 2^28 pixels
        key = mb_key(t.word);
    }
    bool owner = false;
    const uint64_t best = reduce(key, thread, owner);
    if (owner) a.tiles[ty * a.tilesX + tx] = (uint32_t)best;
}

// step B.1: the largest-key word over the 3 x 3 tiles around (tx, ty); every address is wave-uniform
CRY_HD uint32_t mb_neighbourhood(const MbGatherArgs& a, uint32_t tx, uint32_t ty)
{
    const uint32_t x0 = tx ? tx - 1u : 0u, x1 = tx + 1u < a.tilesX ? tx + 1u : tx;
    const uint32_t y0 = ty ? ty - 1u : 0u, y1 = ty + 1u < a.tilesY ? ty + 1u : ty;
    uint64_t best = 0u;
    for (uint32_t y = y0; y <= y1; ++y)
        for (uint32_t x = x0; x <= x1; ++x) {
            const uint64_t k = mb_key(a.tiles[y * a.tilesX + x]);
            best = k > best ? k : best;
        }
    return (uint32_t)best;
}

// floor(num / den) for num below 2^16 and den in 1 .. 130, rden = rcp((float)den): the float quotient is within 1e-4 of the true
// one, so its floor is off by at most one either way, which the remainder shows
CRY_HD uint32_t mb_div(uint32_t num, uint32_t den, float rden)
{
    uint32_t q = (uint32_t)((float)num * rden);
    const int32_t r = (int32_t)num - (int32_t)(q * den);
    q = r < 0 ? q - 1u : q;
    q = r >= (int32_t)den ? q + 1u : q;
    return q;
}

// (B[py & 3][px & 3]) of the fog pass's 4 x 4 Bayer matrix (fog_core.hpp)
CRY_HD uint32_t mb_bayer(uint32_t px, uint32_t py)
{
    const uint32_t word = (py & 2u) ? 0x5D7F91B3u : 0x6E4CA280u;
    return (word >> ((((py & 1u) << 2) + (px & 3u)) << 2)) & 15u;
}

// Steps B.3 .. B.5 for one pixel of a tile whose neighbourhood moves: vN = (nx, ny), len(vN) >= kMbStill; `own` is its texel of `in`.
CRY_HD uint32_t mb_gather_pixel(const MbGatherArgs& a, uint32_t px, uint32_t py, uint32_t own, int32_t nx, int32_t ny)
{
    const uint32_t at = py * a.W + px;
    const MbTexel X = load_at<MbTexel>(a.velocity, at * 8u);
    const int32_t lenX = (int32_t)mb_len(X.word);
    const int32_t b = (int32_t)mb_bayer(px, py);
    const int32_t N = (int32_t)a.samples, half = 8 * N, xmax = (int32_t)a.W - 1, ymax = (int32_t)a.H - 1;
    uint32_t Wt = 1u, S0 = own & 255u, S1 = (own >> 8) & 255u, S2 = (own >> 16) & 255u;
    for (int32_t i0 = 0; i0 < N; i0 += (int32_t)kMbBatch) {            // N is wave-uniform
        uint32_t colour[kMbBatch];
        MbTexel Y[kMbBatch];
        int32_t dist2[kMbBatch];
#pragma unroll
        for (uint32_t j = 0; j < kMbBatch; ++j) {
            const int32_t i = i0 + (int32_t)j;
            const bool live = i < N;                                    // N == 2: the batch's last two samples weigh nothing
            const int32_t m = 16 * i + b - half;
            const int32_t ox = live ? (nx * m + half) >> a.shift : 0, oy = live ? (ny * m + half) >> a.shift : 0;
            dist2[j] = live ? 2 * mb_max(mb_abs(ox), mb_abs(oy)) : 0x10000;      // no length reaches it
            const int32_t sx = clampi((int32_t)px + ((ox + 8) >> 4), 0, xmax), sy = clampi((int32_t)py + ((oy + 8) >> 4), 0, ymax);
            const uint32_t sat = mul24((uint32_t)sy, a.W) + (uint32_t)sx;           // below 2^28: byte offsets below 2^31
            Y[j] = load_at<MbTexel>(a.velocity, sat * 8u);
            colour[j] = load_at<uint32_t>(a.in, sat * 4u);
        }
#pragma unroll
        for (uint32_t j = 0; j < kMbBatch; ++j) {
            const int32_t lenY = (int32_t)mb_len(Y[j].word);
            const uint32_t w = (uint32_t)(Y[j].depth <= X.depth && dist2[j] <= lenY) + (uint32_t)(Y[j].depth >= X.depth && dist2[j] <= lenX);
            Wt += w;
            S0 += w * (colour[j] & 255u);
            S1 += w * ((colour[j] >> 8) & 255u);
            S2 += w * ((colour[j] >> 16) & 255u);
        }
    }
    const uint32_t den = 2u * Wt;
    const float rden = rcp_normal((float)den);
    return mb_div(2u * S0 + Wt, den, rden) | (mb_div(2u * S1 + Wt, den, rden) << 8) | (mb_div(2u * S2 + Wt, den, rden) << 16) | (own & 0xFF000000u);
}

// One thread of the gather workgroup of tile (tx, ty): no thread waits for another.  The pixel's own texel is loaded before the tile
// words are looked at -- both outcomes need it, and a still tile then costs one memory round trip, not two: its threads store what
// they hold.  A thread outside the frame or the row range reads texel 0 (valid memory) and stores nothing.
CRY_HD void mb_gather_thread(const MbGatherArgs& a, uint32_t tx, uint32_t ty, uint32_t thread)
{
    const uint32_t px = tx * kMbTile + (thread & (kMbTile - 1u)), py = ty * kMbTile + (thread >> 4);
    const bool inside = px < a.W && py >= a.row0 && py < a.rowEnd;
    const uint32_t at = inside ? py * a.W + px : 0u;
    const uint32_t own = a.in[at];
    const uint32_t vN = mb_neighbourhood(a, tx, ty);
    if (!inside) return;
    a.out[at] = mb_len(vN) < kMbStill ? own : mb_gather_pixel(a, px, py, own, mb_qx(vN), mb_qy(vN));         // the condition is wave-uniform
}

}  // namespace cry
