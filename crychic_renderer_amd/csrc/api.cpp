// api.cpp -- the extern "C" surface of libcrychic_hip.so (include/crychic_hip.h): argument validation, the
// stream-ordered pass sequencing of Ssao::ComputeSsao (Ssao.cpp:185-243) and of the hot part of
// CRYCHIC::Draw (CRYCHIC.cpp:220-221,238-279), and per-pass HIP-event timing.  No CPU compute path exists
// here: every compute entry point needs a context bound to a HIP device.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <utility>
#include <new>
#include "crychic_hip.h"
#include "kernels.hpp"
#include "light_core.hpp"
#include "light_bind.hpp"
#include "ssao_core.hpp"
#include "blur_tiles.hpp"
#include "raster_core.hpp"
#include "cube_mips_core.hpp"
#include "post_aa_core.hpp"
#include "fog_core.hpp"
#include "ssr_core.hpp"
#include "ssr_gloss_core.hpp"
#include "dof_core.hpp"
#include "bloom_core.hpp"
#include "grade_core.hpp"
#include "sharpen_core.hpp"
#include "taa_core.hpp"
#include "taa_upscale_core.hpp"
#include "motion_blur_core.hpp"
#include "decal_core.hpp"
#include "sky_core.hpp"
#include "internal.hpp"

namespace {
thread_local char g_err[512] = "";
}

namespace cry {
// shared with comm.cpp (internal.hpp): records the thread-local message behind crychic_last_error()
int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace cry

namespace {
using cry::fail;

#define CRY_HIP(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(CRYCHIC_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// The size bound of every pass: 2^28 pixels (32-bit texel indices, plane offsets below 2^30), fewer than 2^20 columns where
// `columns`, and at most maxRows rows (a pass's pixel rows per workgroup row x 65535, grid.y <= 65535; 0: no such limit).
int check_extent(const char* what, uint32_t W, uint32_t H, bool columns, uint32_t maxRows)
{
    if ((uint64_t)W * H <= (1ull << 28) && !(columns && W >= (1u << 20)) && !(maxRows && H > maxRows)) return 0;
    char limits[48] = "";
    if (maxRows) snprintf(limits, sizeof limits, columns ? ", 2^20 columns or %u rows" : " or %u rows", maxRows);
    return fail(CRYCHIC_E_UNSUPPORTED, "%s %ux%u exceeds 2^28 pixels%s", what, W, H, limits);
}

int check_dims(uint32_t W, uint32_t H)
{
    if (W == 0 || H == 0 || (W & 1u) || (H & 1u))
        return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero and even (half-res maps are W/2 x H/2)", W, H);
    return check_extent("frame", W, H, true, 4u * 65535u);      // the lighting pass: 4 pixel rows per workgroup row
}

// Rows [row0, row0 + rows) inside `limit` rows, and at least minRows of them; `fmt` names what they are rows of.
constexpr const char* kAmbientRows = "rows [%u,+%u) outside the %u-row ambient map";
constexpr const char* kFrameRows = "rows [%u,+%u) outside the %u-row frame";
constexpr const char* kTargetRows = "G-buffer rows [%u,+%u) outside the %u-row target";
int check_rows(const char* fmt, uint32_t row0, uint32_t rows, uint32_t limit, uint32_t minRows = 0u)
{
    if (rows < minRows || row0 > limit || rows > limit - row0) return fail(CRYCHIC_E_INVALID_ARG, fmt, row0, rows, limit);
    return 0;
}

// CRYCHIC_LIGHT_CUBE_LEVELS announces at most 15 levels, and a chain ends at 1 x 1 at the latest.
int check_cube_levels(uint32_t levels, uint32_t dim, uint32_t minLevels)
{
    const uint32_t full = cry::cube_full_levels(dim) < 15u ? cry::cube_full_levels(dim) : 15u;
    if (levels < minLevels || levels > full)
        return fail(CRYCHIC_E_INVALID_ARG, "%u cube map levels, a %u-texel face has at most %u", levels, dim, full);
    return 0;
}

bool ranges_overlap(uintptr_t a, size_t aBytes, uintptr_t b, size_t bBytes) { return a < b + bBytes && b < a + aBytes; }

}  // namespace


namespace {

int bind(crychic_ctx* ctx)
{
    if (!ctx) return fail(CRYCHIC_E_INVALID_ARG, "null context");
    CRY_HIP(hipSetDevice(ctx->device));
    return 0;
}

// Frame stamps mark what the SSAO pass of one frame wrote into the (caller-owned) edge workspace.  They come from one
// process-wide counter, so two contexts -- or a context re-created over recycled memory -- never issue the same value.
std::atomic<uint32_t> g_frameStamp{ 0x5EED0000u };
uint32_t next_stamp()
{
    uint32_t s;
    do { s = g_frameStamp.fetch_add(1u, std::memory_order_relaxed) + 1u; } while (s == 0u);      // never 0
    return s;
}

using cry::clamp_rows;

int ssao_compute_impl(const crychic_ssao_constants* cb, const void* normal, const uint32_t* depth,
                      const uint8_t* randvec, uint16_t* ambient0, uint16_t* ambient1, void* edge, uint32_t W,
                      uint32_t H, int blurCount, uint32_t row0, uint32_t rows, hipStream_t stream, hipEvent_t afterSsao, crychic_ctx* ctx)
{
    const uint32_t h2 = H / 2;
    if (int rc = check_rows(kAmbientRows, row0, rows, h2)) return rc;
    if (blurCount < 0) return fail(CRYCHIC_E_INVALID_ARG, "blurCount %d < 0", blurCount);
    if (blurCount > 0 && (!ambient1 || !edge)) return fail(CRYCHIC_E_INVALID_ARG, "blurCount > 0 needs ambient1 and the edge workspace");
    // rows, planes and launches: blur_tiles.hpp "the launch plan"
    uint32_t r0, rn;
    cry::blur_chain_ssao_rows(blurCount, row0, rows, h2, &r0, &rn);
    uint16_t* planes[2] = { ambient0, ambient1 };
    // With a workspace at hand the depth plane is re-laid once per frame as decoded pairs -- for the rows of this call and a margin:
    // the taps of a row reach far up and down the frame, and the few that leave the margin take the raw plane -- and
    // the taps gather from that; its cost is part of the SSAO pass.
    const uint32_t stamp = next_stamp();
    // (gathering from the raw D24 plane with the coarse maps alone was measured too: the depth pass drops from 20 to 7 us and the
    // SSAO kernel gains 15: the pairs plane stays)
    // A small strip of a multi-GPU frame (few wavefronts: its SSAO pass is a chain of round trips, not arithmetic) skips the pairs plane:
    // the depth pass writes the coarse maps only and the taps gather from the raw plane -- the same bits, 1.6 us less for a 1/8 strip of
    // the 4K frame, where the whole frame gains 8 us from the plane (profiles/r04_experiments.txt).  CRYCHIC_STRIP_PAIRS=1: always the plane.
    static const bool stripPairs = getenv("CRYCHIC_STRIP_PAIRS") != nullptr;
    const bool smallStrip = rn < h2 && ((W / 2u + 63u) / 64u) * rn < 4096u;
    const bool usePairs = edge != nullptr && (stripPairs || !smallStrip);
    if (edge) CRY_HIP(cry::launch_depth_pairs(*cb, depth, edge, W, H, stamp, usePairs, r0, rn, stream));
    CRY_HIP(cry::launch_ssao(*cb, normal, depth, randvec, planes[cry::blur_chain_ssao_plane(blurCount)], edge, W, H, r0, rn, true, usePairs,
                             edge ? stamp : 0u, stream));
    if (afterSsao) CRY_HIP(hipEventRecord(afterSsao, stream));
    static const bool perIteration = getenv("CRYCHIC_BLUR_PER_ITERATION") != nullptr;      // the round-3 launch plan, kept for A / B runs
    for (int i = 0; i < cry::blur_chain_launches(blurCount); ++i) {
        const cry::BlurStep s = cry::blur_chain_step(blurCount, row0, rows, h2, i);
        if (i == 0)      // a pixel's value after the frame's sweeps depends on inputs within 5 pixels per iteration
            CRY_HIP(cry::launch_blur_pair(*cb, edge, planes[s.in], planes[s.out], W, H, s.row0, s.rows, blurCount > 1, stamp, 5 * blurCount, r0, rn, stream));
        else if (perIteration || blurCount - 1 > 8)
            CRY_HIP(cry::launch_blur_replay(*cb, edge, planes[s.in], planes[s.out], W, H, s.row0, s.rows, stamp, stream));
        else {           // iterations 1 .. blurCount - 1 as one launch with per-tile dependencies
            CRY_HIP(cry::launch_blur_replay_chain(*cb, edge, planes[0], planes[1], W, H, blurCount, row0, rows, stamp, stream));
            if (ctx) {
                ctx->chainStatus = cry::edge_plane_carve(edge, W, H).progress + (size_t)cry::blur_tiles_x(W) * cry::blur_tiles_y(H);
                ctx->chainTag = ((unsigned long long)stamp << 8) | 255ull;
            }
            break;
        }
    }
    return 0;
}

int fill_light_params(cry::LightParams& P, const crychic_pass_constants* cb, const uint32_t* const shadow[4],
                      uint32_t shadowDim, uint32_t cubeDim, uint32_t W, uint32_t H, int numDirLights,
                      float pcfSearchRadius, uint32_t flags)
{
    if (numDirLights < 0 || numDirLights > CRYCHIC_MAX_LIGHTS)
        return fail(CRYCHIC_E_INVALID_ARG, "numDirLights %d outside [0,%d]", numDirLights, CRYCHIC_MAX_LIGHTS);
    if (shadowDim < 2 || cubeDim < 2 || shadowDim > 16384 || cubeDim > 8192)
        return fail(CRYCHIC_E_INVALID_ARG, "shadowDim %u / cubeDim %u outside [2, 16384] / [2, 8192]", shadowDim, cubeDim);
    if (!(pcfSearchRadius >= 0.0f)) return fail(CRYCHIC_E_INVALID_ARG, "pcfSearchRadius must be >= 0");
    for (int i = 0; i < 4; ++i)
        if (!shadow[i]) return fail(CRYCHIC_E_INVALID_ARG, "shadow cascade %d is null", i);
    const uint32_t levels = (flags >> 16) & 15u;          // CRYCHIC_LIGHT_CUBE_LEVELS; 0: no chain
    if (int rc = check_cube_levels(levels, cubeDim, 0u)) return rc;
    if ((flags & CRYCHIC_LIGHT_CUBE_GLOSS) && levels < 2u)
        return fail(CRYCHIC_E_INVALID_ARG, "CRYCHIC_LIGHT_CUBE_GLOSS needs a chain: CRYCHIC_LIGHT_CUBE_LEVELS(n) with n > 1");
    cry::bind_light_params(P, *cb, shadow, shadowDim, cubeDim, W, H, numDirLights, pcfSearchRadius, flags);
    return 0;
}

// bind_local_lights' point and spot lights and spot shadows.
int bind_spot_lights(cry::LightParams& P, cry::SpotShadows& S, const crychic_pass_constants* cb, const crychic_light* points,
                     uint32_t nPoints, const crychic_light* spots, uint32_t nSpots, const crychic_spot_shadows* d)
{
    if (nPoints > cry::kMaxPointLights || (nPoints && !points))
        return fail(CRYCHIC_E_INVALID_ARG, "numPointLights %u (max %u) / null light buffer", nPoints, cry::kMaxPointLights);
    if (nSpots > cry::kMaxSpotLights || (nSpots && !spots))
        return fail(CRYCHIC_E_INVALID_ARG, "numSpotLights %u (max %u) / null spot light buffer", nSpots, cry::kMaxSpotLights);
    cry::bind_point_lights(P, points, nPoints);
    const uint32_t count = d ? d->count : 0u;
    if (count > CRYCHIC_MAX_SPOT_SHADOWS || count > nSpots)
        return fail(CRYCHIC_E_INVALID_ARG, "spot shadows: count %u (max %u, and at most numSpotLights %u)", count,
                    (unsigned)CRYCHIC_MAX_SPOT_SHADOWS, nSpots);
    if (count && (d->dim < 2 || d->dim > CRYCHIC_MAX_SPOT_SHADOW_DIM))          // 2 texels at least, as the cascades: a footprint row is one pair
        return fail(CRYCHIC_E_INVALID_ARG, "spot shadows: dim %u (2 .. %u)", d->dim, (unsigned)CRYCHIC_MAX_SPOT_SHADOW_DIM);
    for (uint32_t k = 0; k < count; ++k)
        if (!d->maps[k]) return fail(CRYCHIC_E_INVALID_ARG, "spot shadows: null map %u of %u", k, count);
    cry::bind_spot_shadows(S, *cb, d ? d->maps : nullptr, count, d ? d->dim : 0u);
    return 0;
}

// The local lights of one lighting pass (every crychic_deferred_light* entry and the hot paths): at most 1024 point and 1024 spot
// lights, each from a device buffer when there are any, into P; the descriptor's first `count` maps and ShadowTransforms[4 + k]
// into S; the point descriptor's first `count` maps and transposed shadowProj into PS.  A NULL descriptor or count 0 leaves
// S.count = 0 / PS.count = 0: the kernels without those shadows.  Touches neither P's other fields nor cb.
int bind_local_lights(cry::LightParams& P, cry::SpotShadows& S, cry::PointShadows& PS, const crychic_pass_constants* cb,
                      const crychic_light* points, uint32_t nPoints, const crychic_light* spots, uint32_t nSpots,
                      const crychic_spot_shadows* d, const crychic_point_shadows* pd)
{
    if (int rc = bind_spot_lights(P, S, cb, points, nPoints, spots, nSpots, d)) return rc;
    const uint32_t count = pd ? pd->count : 0u;
    if (count > CRYCHIC_MAX_POINT_SHADOWS || count > nPoints)
        return fail(CRYCHIC_E_INVALID_ARG, "point shadows: count %u (max %u, and at most numPointLights %u)", count,
                    (unsigned)CRYCHIC_MAX_POINT_SHADOWS, nPoints);
    if (count && (pd->dim < CRYCHIC_MIN_POINT_SHADOW_DIM || pd->dim > CRYCHIC_MAX_SPOT_SHADOW_DIM))     // the widened faces need 2 texels of rim
        return fail(CRYCHIC_E_INVALID_ARG, "point shadows: dim %u (%u .. %u)", pd->dim, (unsigned)CRYCHIC_MIN_POINT_SHADOW_DIM,
                    (unsigned)CRYCHIC_MAX_SPOT_SHADOW_DIM);
    for (uint32_t k = 0; k < count; ++k)
        if (!pd->maps[k]) return fail(CRYCHIC_E_INVALID_ARG, "point shadows: null map %u of %u", k, count);
    cry::bind_point_shadows(PS, pd ? pd->maps : nullptr, pd ? &pd->shadowProj[0][0] : nullptr, count, pd ? pd->dim : 0u);
    return 0;
}

// CRYCHIC_LIGHT_AMBIENT_SH: the lookup it goes with and the environment tail behind the cube map, before anything is enqueued.
int check_ambient_sh(uint32_t flags, const uint8_t* cube, uint32_t cubeDim)
{
    switch (cry::ambient_sh_check(flags, cube, cubeDim)) {
    case cry::AmbientShCheck::DerivativeChain:
        return fail(CRYCHIC_E_UNSUPPORTED, "CRYCHIC_LIGHT_AMBIENT_SH with a derivative-LOD chain: use no chain, or CRYCHIC_LIGHT_CUBE_LEVELS(n) with CRYCHIC_LIGHT_CUBE_GLOSS");
    case cry::AmbientShCheck::NullCube: return fail(CRYCHIC_E_INVALID_ARG, "CRYCHIC_LIGHT_AMBIENT_SH: null cube map");
    case cry::AmbientShCheck::MisalignedTail:
        return fail(CRYCHIC_E_INVALID_ARG, "CRYCHIC_LIGHT_AMBIENT_SH: the environment tail at cube_dev + %zu is not 4-byte aligned",
                    cry::ambient_sh_offset(cubeDim, (flags >> 16) & 15u));
    default: return 0;
    }
}

// CRYCHIC_LIGHT_ENV_BRDF: the lookup it goes with and the table behind the environment tail, before anything is enqueued.
int check_env_brdf(uint32_t flags, const uint8_t* cube, uint32_t cubeDim)
{
    const cry::EnvBrdfCheck c = cry::env_brdf_check(flags, cube, cubeDim);
    if (c == cry::EnvBrdfCheck::Ok) return 0;
    return fail(CRYCHIC_E_INVALID_ARG, cry::env_brdf_check_message(c), cry::env_brdf_offset(cubeDim, (flags >> 16) & 15u));
}

// CRYCHIC_LIGHT_CUBE_PARALLAX: the lookup it goes with and the probe volume in the environment tail, before anything is enqueued.
int check_parallax(uint32_t flags, const uint8_t* cube, uint32_t cubeDim)
{
    const cry::ParallaxCheck c = cry::parallax_check(flags, cube, cubeDim);
    if (c == cry::ParallaxCheck::Ok) return 0;
    return fail(CRYCHIC_E_INVALID_ARG, cry::parallax_check_message(c), cry::parallax_probe_offset(cubeDim, (flags >> 16) & 15u));
}

// The three lookups behind the cube map, in the order their refusals take precedence.
int check_environment(uint32_t flags, const uint8_t* cube, uint32_t cubeDim)
{
    if (int rc = check_ambient_sh(flags, cube, cubeDim)) return rc;
    if (int rc = check_env_brdf(flags, cube, cubeDim)) return rc;
    return check_parallax(flags, cube, cubeDim);
}

// With a mip chain the level of detail comes from 2 x 2 pixel quads: a call's rows have to be whole quad rows.  Not so with
// CRYCHIC_LIGHT_CUBE_GLOSS, where it comes from the pixel's roughness.
int check_chain_rows(const cry::LightParams& P, uint32_t row0, uint32_t rows, uint32_t H)
{
    if (P.cubeLevels > 1u && !(P.flags & CRYCHIC_LIGHT_CUBE_GLOSS) && ((row0 & 1u) || ((rows & 1u) && row0 + rows != H)))
        return fail(CRYCHIC_E_INVALID_ARG, "rows [%u,+%u): with a cube map mip chain a call covers whole pixel quads (even row0; even rows unless they end the frame)", row0, rows);
    return 0;
}

// Every crychic_deferred_light* entry: the lights the entry does not take are null / 0.
int deferred_light_impl(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev, const float* g2_dev,
                        const uint32_t* depth_dev, const uint16_t* ambient_dev, const uint32_t* const shadow_dev[4], uint32_t shadowDim,
                        const uint8_t* cube_dev, uint32_t cubeDim, uint8_t* out_rgba8_dev, float* radiance_out_dev, uint32_t W, uint32_t H,
                        uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags, const crychic_light* point_lights_dev,
                        uint32_t numPointLights, const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                        const crychic_spot_shadows* spotShadows, const crychic_point_shadows* pointShadows, void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_dims(W, H)) return rc;
    if (!cb || !g0_dev || !g1_dev || !g2_dev || !depth_dev || !shadow_dev || !cube_dev || !out_rgba8_dev)
        return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    cry::LightParams P;
    cry::SpotShadows S;
    cry::PointShadows PS;
    if (int rc = bind_local_lights(P, S, PS, cb, point_lights_dev, numPointLights, spot_lights_dev, numSpotLights, spotShadows,
                                   pointShadows)) return rc;
    if (int rc = fill_light_params(P, cb, shadow_dev, shadowDim, cubeDim, W, H, numDirLights, pcfSearchRadius, flags)) return rc;
    if (int rc = check_environment(flags, cube_dev, cubeDim)) return rc;
    if (int rc = check_chain_rows(P, row0, rows, H)) return rc;
    CRY_HIP(cry::launch_light(P, g0_dev, g1_dev, g2_dev, depth_dev, ambient_dev, cube_dev, out_rgba8_dev, radiance_out_dev,
                              row0, rows, (hipStream_t)stream, spot_lights_dev, numSpotLights, &S, &PS));
    return 0;
}

}  // namespace

extern "C" {

const char* crychic_last_error(void) { return g_err; }
const char* crychic_version(void) { return "crychic-hip 0.1 (gfx950)"; }

int crychic_ctx_create(int device_ordinal, crychic_ctx** out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(CRYCHIC_E_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= count)
        return fail(CRYCHIC_E_NO_DEVICE, "device ordinal %d outside [0,%d)", device_ordinal, count);
    CRY_HIP(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    CRY_HIP(hipGetDeviceProperties(&prop, device_ordinal));
    crychic_ctx* ctx = new (std::nothrow) crychic_ctx();
    if (!ctx) return fail(CRYCHIC_E_HIP, "out of host memory");
    ctx->device = device_ordinal;
    snprintf(ctx->name, sizeof ctx->name, "%s %s", prop.gcnArchName, prop.name);
    ctx->profiling = false;
    ctx->times_valid = false;
    ctx->rasterStatus = nullptr;
    ctx->chainStatus = nullptr;
    ctx->chainTag = 0ull;
    for (auto& ev : ctx->ev) {
        hipError_t ee = hipEventCreate(&ev);
        if (ee != hipSuccess) { delete ctx; return fail(CRYCHIC_E_HIP, "hipEventCreate failed: %s", hipGetErrorString(ee)); }
    }
    *out = ctx;
    return 0;
}

void crychic_ctx_destroy(crychic_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (auto& ev : ctx->ev) (void)hipEventDestroy(ev);
    delete ctx;
}

const char* crychic_ctx_device_name(crychic_ctx* ctx) { return ctx ? ctx->name : nullptr; }

size_t crychic_edge_plane_bytes(uint32_t W, uint32_t H) { return cry::edge_plane_bytes(W, H); }

int crychic_ssao(crychic_ctx* ctx, const crychic_ssao_constants* cb, const void* normal_dev, const uint32_t* depth_dev,
                 const uint8_t* randvec_dev, uint16_t* ambient_out_dev, void* edge_dev, uint32_t W, uint32_t H,
                 uint32_t row0, uint32_t rows, void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_dims(W, H)) return rc;
    if (!cb || !normal_dev || !depth_dev || !randvec_dev || !ambient_out_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (int rc = check_rows(kAmbientRows, row0, rows, H / 2)) return rc;
    const uint32_t stamp = next_stamp();
    const bool usePairs = edge_dev != nullptr;
    if (edge_dev) CRY_HIP(cry::launch_depth_pairs(*cb, depth_dev, edge_dev, W, H, stamp, usePairs, row0, rows, (hipStream_t)stream));
    CRY_HIP(cry::launch_ssao(*cb, normal_dev, depth_dev, randvec_dev, ambient_out_dev, edge_dev, W, H, row0, rows, true, usePairs,
                             edge_dev ? stamp : 0u, (hipStream_t)stream));
    return 0;
}

int crychic_ssao_edges(crychic_ctx* ctx, const crychic_ssao_constants* cb, const void* normal_dev,
                       const uint32_t* depth_dev, void* edge_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                       void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_dims(W, H)) return rc;
    if (!cb || !normal_dev || !depth_dev || !edge_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (int rc = check_rows(kAmbientRows, row0, rows, H / 2)) return rc;
    CRY_HIP(cry::launch_ssao(*cb, normal_dev, depth_dev, nullptr, nullptr, edge_dev, W, H, row0, rows, false, false, 0u, (hipStream_t)stream));
    return 0;
}

int crychic_ssao_blur(crychic_ctx* ctx, const crychic_ssao_constants* cb, const void* edge_dev,
                      const uint16_t* ambient_in_dev, uint16_t* ambient_out_dev, uint32_t W, uint32_t H, int horizontal,
                      uint32_t row0, uint32_t rows, void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_dims(W, H)) return rc;
    if (!cb || !edge_dev || !ambient_in_dev || !ambient_out_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (ambient_in_dev == ambient_out_dev) return fail(CRYCHIC_E_INVALID_ARG, "blur cannot run in place (the reference ping-pongs, Ssao.cpp:253-266)");
    if (int rc = check_rows(kAmbientRows, row0, rows, H / 2)) return rc;
    CRY_HIP(cry::launch_blur(*cb, edge_dev, ambient_in_dev, ambient_out_dev, W, H, horizontal != 0, row0, rows, (hipStream_t)stream));
    return 0;
}

int crychic_ssao_compute(crychic_ctx* ctx, const crychic_ssao_constants* cb, const void* normal_dev,
                         const uint32_t* depth_dev, const uint8_t* randvec_dev, uint16_t* ambient0_dev,
                         uint16_t* ambient1_dev, void* edge_dev, uint32_t W, uint32_t H, int blurCount, uint32_t row0,
                         uint32_t rows, void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (int rc = check_dims(W, H)) return rc;
    if (!cb || !normal_dev || !depth_dev || !randvec_dev || !ambient0_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    return ssao_compute_impl(cb, normal_dev, depth_dev, randvec_dev, ambient0_dev, ambient1_dev, edge_dev, W, H,
                             blurCount, row0, rows, (hipStream_t)stream, nullptr, ctx);
}

int crychic_deferred_light(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev,
                           const float* g2_dev, const uint32_t* depth_dev, const uint16_t* ambient_dev,
                           const uint32_t* const shadow_dev[4], uint32_t shadowDim, const uint8_t* cube_dev,
                           uint32_t cubeDim, uint8_t* out_rgba8_dev, float* radiance_out_dev, uint32_t W, uint32_t H,
                           uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                           void* stream)
{
    return deferred_light_impl(ctx, cb, g0_dev, g1_dev, g2_dev, depth_dev, ambient_dev, shadow_dev, shadowDim, cube_dev, cubeDim, out_rgba8_dev,
                               radiance_out_dev, W, H, row0, rows, numDirLights, pcfSearchRadius, flags, nullptr, 0u, nullptr, 0u, nullptr, nullptr, stream);
}

int crychic_deferred_light_points(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev,
                                  const float* g2_dev, const uint32_t* depth_dev, const uint16_t* ambient_dev,
                                  const uint32_t* const shadow_dev[4], uint32_t shadowDim, const uint8_t* cube_dev,
                                  uint32_t cubeDim, uint8_t* out_rgba8_dev, float* radiance_out_dev, uint32_t W, uint32_t H,
                                  uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                                  const crychic_light* point_lights_dev, uint32_t numPointLights, void* stream)
{
    return deferred_light_impl(ctx, cb, g0_dev, g1_dev, g2_dev, depth_dev, ambient_dev, shadow_dev, shadowDim, cube_dev, cubeDim, out_rgba8_dev,
                               radiance_out_dev, W, H, row0, rows, numDirLights, pcfSearchRadius, flags, point_lights_dev, numPointLights,
                               nullptr, 0u, nullptr, nullptr, stream);
}

int crychic_deferred_light_spots(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev,
                                 const float* g2_dev, const uint32_t* depth_dev, const uint16_t* ambient_dev,
                                 const uint32_t* const shadow_dev[4], uint32_t shadowDim, const uint8_t* cube_dev,
                                 uint32_t cubeDim, uint8_t* out_rgba8_dev, float* radiance_out_dev, uint32_t W, uint32_t H,
                                 uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                                 const crychic_light* point_lights_dev, uint32_t numPointLights,
                                 const crychic_light* spot_lights_dev, uint32_t numSpotLights, void* stream)
{
    return deferred_light_impl(ctx, cb, g0_dev, g1_dev, g2_dev, depth_dev, ambient_dev, shadow_dev, shadowDim, cube_dev, cubeDim, out_rgba8_dev,
                               radiance_out_dev, W, H, row0, rows, numDirLights, pcfSearchRadius, flags, point_lights_dev, numPointLights,
                               spot_lights_dev, numSpotLights, nullptr, nullptr, stream);
}

int crychic_deferred_light_spots_shadowed(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev,
                                          const float* g2_dev, const uint32_t* depth_dev, const uint16_t* ambient_dev,
                                          const uint32_t* const shadow_dev[4], uint32_t shadowDim, const uint8_t* cube_dev,
                                          uint32_t cubeDim, uint8_t* out_rgba8_dev, float* radiance_out_dev, uint32_t W, uint32_t H,
                                          uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                                          const crychic_light* point_lights_dev, uint32_t numPointLights,
                                          const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                          const crychic_spot_shadows* spotShadows, void* stream)
{
    return deferred_light_impl(ctx, cb, g0_dev, g1_dev, g2_dev, depth_dev, ambient_dev, shadow_dev, shadowDim, cube_dev, cubeDim, out_rgba8_dev,
                               radiance_out_dev, W, H, row0, rows, numDirLights, pcfSearchRadius, flags, point_lights_dev, numPointLights,
                               spot_lights_dev, numSpotLights, spotShadows, nullptr, stream);
}

int crychic_deferred_light_point_shadows(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev,
                                         const float* g2_dev, const uint32_t* depth_dev, const uint16_t* ambient_dev,
                                         const uint32_t* const shadow_dev[4], uint32_t shadowDim, const uint8_t* cube_dev,
                                         uint32_t cubeDim, uint8_t* out_rgba8_dev, float* radiance_out_dev, uint32_t W, uint32_t H,
                                         uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                                         const crychic_light* point_lights_dev, uint32_t numPointLights,
                                         const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                         const crychic_spot_shadows* spotShadows, const crychic_point_shadows* pointShadows, void* stream)
{
    return deferred_light_impl(ctx, cb, g0_dev, g1_dev, g2_dev, depth_dev, ambient_dev, shadow_dev, shadowDim, cube_dev, cubeDim, out_rgba8_dev,
                               radiance_out_dev, W, H, row0, rows, numDirLights, pcfSearchRadius, flags, point_lights_dev, numPointLights,
                               spot_lights_dev, numSpotLights, spotShadows, pointShadows, stream);
}

}  // extern "C"

// crychic_draw_hot_path with the lighting pass issued as `nparts` consecutive row ranges of the strip (even-aligned, the
// crychic_strip_rows cut of the strip's rows); after(user, part, row0, rows) runs behind part's launch -- comm.cpp hangs that
// part's exchange there (crychic_draw_hot_path_shared).  nparts == 1, after == nullptr is crychic_draw_hot_path itself.
int cry::hot_path_parts(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                        const crychic_frame_desc* f, hipStream_t stream, uint32_t nparts, cry::PartHook after, void* user,
                        const cry::SpotLightArgs& spots)
{
    if (int rc = bind(ctx)) return rc;
    if (!ssaoCB || !passCB || !f) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (int rc = check_dims(f->W, f->H)) return rc;
    const uint32_t W = f->W, H = f->H;
    if (f->row0 > H || f->rows > H - f->row0 || (f->row0 & 1u) || ((f->rows & 1u) && f->row0 + f->rows != H))
        return fail(CRYCHIC_E_INVALID_ARG, "strip [%u,+%u) must lie inside the frame and start on an even row", f->row0, f->rows);
    if (!f->depth_dev || !f->g0_dev || !f->g1_dev || !f->g2_dev || !f->cube_dev || !f->out_rgba8_dev)
        return fail(CRYCHIC_E_INVALID_ARG, "null plane in frame descriptor");
    const bool ssaoOn = f->blurCount >= 0;
    if (ssaoOn && (!f->normal_dev || !f->randvec_dev || !f->ambient0_dev)) return fail(CRYCHIC_E_INVALID_ARG, "SSAO planes missing");
    if (nparts == 0 || nparts > CRYCHIC_MAX_EXCHANGE_PARTS) return fail(CRYCHIC_E_INVALID_ARG, "nparts %u (1 .. %d)", nparts, CRYCHIC_MAX_EXCHANGE_PARTS);
    cry::LightParams P;
    if (int rc = fill_light_params(P, passCB, f->shadow_dev, f->shadowDim, f->cubeDim, W, H, f->numDirLights,
                                   f->pcfSearchRadius, f->flags)) return rc;
    if (int rc = check_environment(f->flags, f->cube_dev, f->cubeDim)) return rc;
    cry::SpotShadows S;
    cry::PointShadows PS;
    if (int rc = bind_local_lights(P, S, PS, passCB, f->point_lights_dev, f->numPointLights, spots.lights, spots.count, spots.shadows,
                                   spots.pointShadows)) return rc;
    const bool prof = ctx->profiling;
    if (prof) { ctx->times_valid = false; CRY_HIP(hipEventRecord(ctx->ev[0], stream)); }
    if (ssaoOn) {
        // The lighting pass filters the half-res AO map bilinearly at (about) its own pixel centre
        // (DeferredShading.hlsl:40-42): rows row0/2 - 1 .. (row0+rows)/2; keep one more row of slack.
        uint32_t a0, an;
        clamp_rows(H / 2, (int64_t)(f->row0 / 2) - 2, (int64_t)((f->row0 + f->rows + 1) / 2) + 2, &a0, &an);
        if (int rc = ssao_compute_impl(ssaoCB, f->normal_dev, f->depth_dev, f->randvec_dev, f->ambient0_dev,
                                       f->ambient1_dev, f->edge_dev, W, H, f->blurCount, a0, an, stream,
                                       prof ? ctx->ev[1] : nullptr, ctx)) return rc;
    } else if (prof) {
        CRY_HIP(hipEventRecord(ctx->ev[1], stream));
    }
    if (prof) CRY_HIP(hipEventRecord(ctx->ev[2], stream));
    // parts: whole half-res rows each, the last one takes the remainder (and an odd last row of the frame)
    const uint32_t pairs = f->rows / 2u, per = pairs / nparts;
    for (uint32_t p = 0; p < nparts; ++p) {
        const uint32_t r0 = f->row0 + 2u * per * p;
        const uint32_t r1 = (p + 1u == nparts) ? f->row0 + f->rows : r0 + 2u * per;
        if (r1 > r0)
            CRY_HIP(cry::launch_light(P, f->g0_dev, f->g1_dev, f->g2_dev, f->depth_dev, ssaoOn ? f->ambient0_dev : nullptr,
                                      f->cube_dev, f->out_rgba8_dev, nullptr, r0, r1 - r0, stream, spots.lights, spots.count, &S, &PS));
        if (prof && p + 1u == nparts) { CRY_HIP(hipEventRecord(ctx->ev[3], stream)); ctx->times_valid = true; }
        if (after)
            if (int rc = after(user, p, r0, r1 - r0)) return rc;
    }
    return 0;
}

extern "C" {

int crychic_draw_hot_path(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                          const crychic_frame_desc* f, void* stream)
{
    return cry::hot_path_parts(ctx, ssaoCB, passCB, f, (hipStream_t)stream, 1u, nullptr, nullptr, {});
}

int crychic_draw_hot_path_spots(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                                const crychic_frame_desc* f, const crychic_light* spot_lights_dev, uint32_t numSpotLights, void* stream)
{
    return cry::hot_path_parts(ctx, ssaoCB, passCB, f, (hipStream_t)stream, 1u, nullptr, nullptr, { spot_lights_dev, numSpotLights, nullptr });
}

int crychic_draw_hot_path_spots_shadowed(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                                         const crychic_frame_desc* f, const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                         const crychic_spot_shadows* spotShadows, void* stream)
{
    return cry::hot_path_parts(ctx, ssaoCB, passCB, f, (hipStream_t)stream, 1u, nullptr, nullptr, { spot_lights_dev, numSpotLights, spotShadows });
}

int crychic_draw_hot_path_point_shadows(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                                        const crychic_frame_desc* f, const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                        const crychic_spot_shadows* spotShadows, const crychic_point_shadows* pointShadows, void* stream)
{
    return cry::hot_path_parts(ctx, ssaoCB, passCB, f, (hipStream_t)stream, 1u, nullptr, nullptr,
                               { spot_lights_dev, numSpotLights, spotShadows, pointShadows });
}

int crychic_ctx_set_profiling(crychic_ctx* ctx, int enabled)
{
    if (!ctx) return fail(CRYCHIC_E_INVALID_ARG, "null context");
    ctx->profiling = enabled != 0;
    ctx->times_valid = false;
    return 0;
}

int crychic_ctx_last_pass_times(crychic_ctx* ctx, crychic_pass_times* out)
{
    if (int rc = bind(ctx)) return rc;
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    if (!ctx->times_valid) return fail(CRYCHIC_E_INVALID_ARG, "no profiled frame recorded (enable profiling, then draw)");
    CRY_HIP(hipEventSynchronize(ctx->ev[3]));
    CRY_HIP(hipEventElapsedTime(&out->ssao_ms, ctx->ev[0], ctx->ev[1]));
    CRY_HIP(hipEventElapsedTime(&out->blur_ms, ctx->ev[1], ctx->ev[2]));
    CRY_HIP(hipEventElapsedTime(&out->light_ms, ctx->ev[2], ctx->ev[3]));
    CRY_HIP(hipEventElapsedTime(&out->total_ms, ctx->ev[0], ctx->ev[3]));
    return 0;
}

size_t crychic_raster_workspace_bytes(uint64_t triangles, uint32_t W, uint32_t H) { return cry::raster_workspace_bytes(triangles, W, H); }

static int raster_common(crychic_ctx* ctx, cry::RasterPass& p, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                         uint32_t nItems, void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (!passCB || (!items && nItems) || (!p.depth && p.nTargets < 2u) || !p.workspace) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (p.W == 0 || p.H == 0) return fail(CRYCHIC_E_INVALID_ARG, "bad target size %ux%u", p.W, p.H);
    if (int rc = check_extent("target", p.W, p.H, true, 4u * 65535u)) return rc;      // the resolve pass: 4 pixel rows per workgroup row
    for (uint32_t i = 0; i < nItems; ++i) {
        const crychic_draw_item& d = items[i];
        if (d.indexCount % 3u) return fail(CRYCHIC_E_INVALID_ARG, "item %u: indexCount %u is not a triangle list", i, d.indexCount);
        if (d.indexCount && d.instanceCount && (!d.vertices_dev || !d.indices_dev || !d.instances_dev))
            return fail(CRYCHIC_E_INVALID_ARG, "item %u: null buffer", i);
    }
    p.view = passCB->View;
    p.viewProj = passCB->ViewProj;
    p.items = items;
    p.nItems = nItems;
    hipError_t e = cry::launch_raster_pass(p, (hipStream_t)stream);
    if (e == hipSuccess) ctx->rasterStatus = p.statusWord;
    if (e == hipErrorInvalidValue) return fail(CRYCHIC_E_INVALID_ARG, "raster workspace too small (need crychic_raster_workspace_bytes) or too many textures");
    if (e != hipSuccess) return fail(CRYCHIC_E_HIP, "raster pass failed: %s", hipGetErrorString(e));
    return 0;
}

int crychic_raster_status(crychic_ctx* ctx, void* stream, uint32_t* flags)
{
    if (int rc = bind(ctx)) return rc;
    if (!flags) return fail(CRYCHIC_E_INVALID_ARG, "flags is null");
    *flags = 0;
    if (!ctx->rasterStatus) return fail(CRYCHIC_E_INVALID_ARG, "no producer pass has been issued on this context");
    CRY_HIP(hipMemcpyAsync(flags, ctx->rasterStatus, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    CRY_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int crychic_blur_chain_status(crychic_ctx* ctx, void* stream, uint32_t* timed_out)
{
    if (int rc = bind(ctx)) return rc;
    if (!timed_out) return fail(CRYCHIC_E_INVALID_ARG, "timed_out is null");
    *timed_out = 0;
    if (!ctx->chainStatus) return 0;             // no single-launch chain has run on this context
    unsigned long long word = 0;
    CRY_HIP(hipMemcpyAsync(&word, ctx->chainStatus, sizeof word, hipMemcpyDeviceToHost, (hipStream_t)stream));
    CRY_HIP(hipStreamSynchronize((hipStream_t)stream));
    *timed_out = word == ctx->chainTag ? 1u : 0u;
    return 0;
}

// What every producer entry fills in alike: the mode (kernels.hpp), the target's size and depth plane, the workspace.
static cry::RasterPass raster_pass(int mode, uint32_t W, uint32_t H, uint32_t* depth_dev, void* workspace_dev, size_t workspaceBytes)
{
    cry::RasterPass p = {};
    p.mode = mode; p.W = W; p.H = H; p.depth = depth_dev; p.workspace = workspace_dev; p.workspaceBytes = workspaceBytes;
    return p;
}

static cry::RasterPass shadow_pass(uint32_t shadowDim, int depthBias, float slopeScaledDepthBias, uint32_t* shadow_dev, void* workspace_dev,
                                   size_t workspaceBytes)
{
    cry::RasterPass p = raster_pass(0, shadowDim, shadowDim, shadow_dev, workspace_dev, workspaceBytes);
    p.depthBias = depthBias; p.slopeScaledDepthBias = slopeScaledDepthBias;
    return p;
}

int crychic_draw_scene_to_shadow_map(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                                     uint32_t nItems, uint32_t* shadow_dev, uint32_t shadowDim, int depthBias,
                                     float slopeScaledDepthBias, void* workspace_dev, size_t workspaceBytes, void* stream)
{
    cry::RasterPass p = shadow_pass(shadowDim, depthBias, slopeScaledDepthBias, shadow_dev, workspace_dev, workspaceBytes);
    return raster_common(ctx, p, passCB, items, nItems, stream);
}

int crychic_draw_scene_to_shadow_maps(crychic_ctx* ctx, const crychic_pass_constants* passCBs, uint32_t nCascades, const crychic_draw_item* items,
                                      uint32_t nItems, uint32_t* const* shadow_dev, uint32_t shadowDim, int depthBias, float slopeScaledDepthBias,
                                      void* workspace_dev, size_t workspaceBytes, void* stream)
{
    if (!passCBs || !shadow_dev || nCascades < 1u || nCascades > 12u)
        return fail(CRYCHIC_E_INVALID_ARG, "1..12 cascades with their pass constants and targets");
    if (nCascades > 4u) {          // gShadowMap[4..11] (the shadowed spot lights): consecutive fused passes of at most four targets
        for (uint32_t c = 0; c < nCascades; ++c)
            if (!shadow_dev[c]) return fail(CRYCHIC_E_INVALID_ARG, "shadow target %u is null", c);
        for (uint32_t c0 = 0; c0 < nCascades; c0 += 4u) {
            const uint32_t n = nCascades - c0 < 4u ? nCascades - c0 : 4u;
            if (int rc = crychic_draw_scene_to_shadow_maps(ctx, passCBs + c0, n, items, nItems, shadow_dev + c0, shadowDim, depthBias,
                                                           slopeScaledDepthBias, workspace_dev, workspaceBytes, stream))
                return rc;
        }
        return 0;
    }
    if (nCascades == 1u)
        return crychic_draw_scene_to_shadow_map(ctx, passCBs, items, nItems, shadow_dev[0], shadowDim, depthBias, slopeScaledDepthBias, workspace_dev,
                                                workspaceBytes, stream);
    cry::RasterPass p = shadow_pass(shadowDim, depthBias, slopeScaledDepthBias, nullptr, workspace_dev, workspaceBytes);
    p.nTargets = nCascades;
    for (uint32_t c = 0; c < nCascades; ++c) {
        if (!shadow_dev[c]) return fail(CRYCHIC_E_INVALID_ARG, "shadow target %u is null", c);
        p.viewProjN[c] = passCBs[c].ViewProj;
        p.depthN[c] = shadow_dev[c];
    }
    return raster_common(ctx, p, passCBs, items, nItems, stream);
}

int crychic_draw_normals_and_depth(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                                   uint32_t nItems, void* normal_dev, uint32_t* depth_dev, uint32_t W, uint32_t H,
                                   void* workspace_dev, size_t workspaceBytes, void* stream)
{
    if (!normal_dev) return fail(CRYCHIC_E_INVALID_ARG, "null normal target");
    cry::RasterPass p = raster_pass(1, W, H, depth_dev, workspace_dev, workspaceBytes);
    p.normal = normal_dev;
    return raster_common(ctx, p, passCB, items, nItems, stream);
}

// The camera's G-buffer pass behind the five entries below.  `fused`: the entry takes a normal map of its own, which may then not
// be null; with a normal map the pass writes it too (mode 3).  minRows 1: gRows == 0 is refused, not read as the whole target.
static int gbuffer_pass(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items, uint32_t nItems,
                        const crychic_material_data* materials_dev, uint32_t nMaterials, const crychic_texture* textures, uint32_t nTextures,
                        bool fused, void* normal_dev, void* g0_dev, void* g1_dev, void* g2_dev, uint32_t gbufferFlags, uint32_t* depth_dev,
                        uint32_t W, uint32_t H, uint32_t gRow0, uint32_t gRows, uint32_t minRows, void* workspace_dev, size_t workspaceBytes,
                        void* stream)
{
    if ((fused && !normal_dev) || !g0_dev || !g1_dev || !g2_dev)
        return fail(CRYCHIC_E_INVALID_ARG, fused ? "null normal / G-buffer target" : "null G-buffer target");
    if (nTextures && !textures) return fail(CRYCHIC_E_INVALID_ARG, "null texture table");
    if (int rc = check_rows(kTargetRows, gRow0, gRows, H, minRows)) return rc;
    cry::RasterPass p = raster_pass(normal_dev ? 3 : 2, W, H, depth_dev, workspace_dev, workspaceBytes);
    p.normal = normal_dev;
    p.g0 = (float*)g0_dev; p.g1 = (float*)g1_dev; p.g2 = (float*)g2_dev; p.gbufferFlags = gbufferFlags;
    p.materials = materials_dev; p.nMaterials = nMaterials;
    p.textures = reinterpret_cast<const cry::Texture*>(textures); p.nTextures = nTextures;
    p.gRow0 = gRow0; p.gRows = gRows;
    return raster_common(ctx, p, passCB, items, nItems, stream);
}

int crychic_draw_gbuffer(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items, uint32_t nItems,
                         const crychic_material_data* materials_dev, uint32_t nMaterials, const crychic_texture* textures,
                         uint32_t nTextures, float* g0_dev, float* g1_dev, float* g2_dev, uint32_t* depth_dev, uint32_t W, uint32_t H,
                         void* workspace_dev, size_t workspaceBytes, void* stream)
{
    return gbuffer_pass(ctx, passCB, items, nItems, materials_dev, nMaterials, textures, nTextures, false, nullptr, g0_dev, g1_dev, g2_dev, 0u,
                        depth_dev, W, H, 0u, 0u, 0u, workspace_dev, workspaceBytes, stream);
}

int crychic_draw_normals_depth_and_gbuffer(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items, uint32_t nItems,
                                           const crychic_material_data* materials_dev, uint32_t nMaterials, const crychic_texture* textures,
                                           uint32_t nTextures, void* normal_dev, float* g0_dev, float* g1_dev, float* g2_dev, uint32_t* depth_dev,
                                           uint32_t W, uint32_t H, void* workspace_dev, size_t workspaceBytes, void* stream)
{
    return gbuffer_pass(ctx, passCB, items, nItems, materials_dev, nMaterials, textures, nTextures, true, normal_dev, g0_dev, g1_dev, g2_dev, 0u,
                        depth_dev, W, H, 0u, 0u, 0u, workspace_dev, workspaceBytes, stream);
}

int crychic_draw_gbuffer_rows(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items, uint32_t nItems,
                              const crychic_material_data* materials_dev, uint32_t nMaterials, const crychic_texture* textures,
                              uint32_t nTextures, float* g0_dev, float* g1_dev, float* g2_dev, uint32_t* depth_dev, uint32_t W, uint32_t H,
                              uint32_t gRow0, uint32_t gRows, void* workspace_dev, size_t workspaceBytes, void* stream)
{
    return gbuffer_pass(ctx, passCB, items, nItems, materials_dev, nMaterials, textures, nTextures, false, nullptr, g0_dev, g1_dev, g2_dev, 0u,
                        depth_dev, W, H, gRow0, gRows, 1u, workspace_dev, workspaceBytes, stream);
}

int crychic_draw_normals_depth_and_gbuffer_rows(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items, uint32_t nItems,
                                                const crychic_material_data* materials_dev, uint32_t nMaterials, const crychic_texture* textures,
                                                uint32_t nTextures, void* normal_dev, float* g0_dev, float* g1_dev, float* g2_dev, uint32_t* depth_dev,
                                                uint32_t W, uint32_t H, uint32_t gRow0, uint32_t gRows, void* workspace_dev, size_t workspaceBytes,
                                                void* stream)
{
    return gbuffer_pass(ctx, passCB, items, nItems, materials_dev, nMaterials, textures, nTextures, true, normal_dev, g0_dev, g1_dev, g2_dev, 0u,
                        depth_dev, W, H, gRow0, gRows, 1u, workspace_dev, workspaceBytes, stream);
}

size_t crychic_gbuffer_plane_bytes(uint32_t W, uint32_t H, uint32_t flags, int plane)
{
    if (plane < 0 || plane > 2) return 0;
    return (size_t)W * H * ((flags & (CRYCHIC_GBUFFER_G0_F16 << plane)) ? 8u : 16u);
}

int crychic_draw_gbuffer_formats(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items, uint32_t nItems,
                                 const crychic_material_data* materials_dev, uint32_t nMaterials, const crychic_texture* textures,
                                 uint32_t nTextures, void* normal_dev, void* g0_dev, void* g1_dev, void* g2_dev, uint32_t gbufferFlags,
                                 uint32_t* depth_dev, uint32_t W, uint32_t H, uint32_t gRow0, uint32_t gRows, void* workspace_dev,
                                 size_t workspaceBytes, void* stream)
{
    if (gbufferFlags & ~CRYCHIC_GBUFFER_F16_MASK)
        return fail(CRYCHIC_E_INVALID_ARG, "gbufferFlags 0x%x: bits outside CRYCHIC_GBUFFER_G0_F16 | G1_F16 | G2_F16", gbufferFlags);
    return gbuffer_pass(ctx, passCB, items, nItems, materials_dev, nMaterials, textures, nTextures, false, normal_dev, g0_dev, g1_dev, g2_dev,
                        gbufferFlags, depth_dev, W, H, gRow0, gRows, 0u, workspace_dev, workspaceBytes, stream);
}

size_t crychic_cube_chain_bytes(uint32_t dim, uint32_t levels)
{
    size_t bytes = 0;
    for (uint32_t k = 0; k < levels; ++k) bytes += cry::cube_level_texels(cry::cube_mip_dim(dim, k)) * 4u;
    return bytes;
}

int crychic_generate_cube_mips(crychic_ctx* ctx, uint8_t* chain_dev, uint32_t dim, uint32_t levels, void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (!chain_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (dim == 0) return fail(CRYCHIC_E_INVALID_ARG, "cube map face size 0");
    if (dim > 32768u) return fail(CRYCHIC_E_UNSUPPORTED, "cube map face size %u exceeds 32768", dim);
    if (int rc = check_cube_levels(levels, dim, 1u)) return rc;
    if (reinterpret_cast<uintptr_t>(chain_dev) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "cube map chain is not 4-byte aligned");
    CRY_HIP(cry::launch_cube_mips(chain_dev, dim, levels, (hipStream_t)stream));
    return 0;
}

int crychic_prefilter_cube_chain(crychic_ctx* ctx, const uint8_t* src_chain_dev, uint8_t* dst_chain_dev, uint32_t dim, uint32_t levels,
                                 void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (!src_chain_dev || !dst_chain_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (dim == 0) return fail(CRYCHIC_E_INVALID_ARG, "cube map face size 0");
    // the chain sampler addresses texels by 32-bit byte offsets, as it does in the lighting pass (cubeDim <= 8192 there)
    if (dim > 8192u) return fail(CRYCHIC_E_UNSUPPORTED, "cube map face size %u exceeds 8192", dim);
    if (int rc = check_cube_levels(levels, dim, 1u)) return rc;
    const uintptr_t s = reinterpret_cast<uintptr_t>(src_chain_dev), d = reinterpret_cast<uintptr_t>(dst_chain_dev);
    if ((s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "cube map chain is not 4-byte aligned");
    const size_t bytes = crychic_cube_chain_bytes(dim, levels);
    if (ranges_overlap(s, bytes, d, bytes)) return fail(CRYCHIC_E_INVALID_ARG, "the source and destination chains overlap");
    CRY_HIP(cry::launch_cube_prefilter(src_chain_dev, dst_chain_dev, dim, levels, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_AA_MAX_SEARCH == cry::kAaMaxSearch && sizeof(crychic_aa_params) == sizeof(cry::PostAaParams), "post_aa_core.hpp mirrors the ABI");

int crychic_aa_default_params(crychic_aa_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    out->absMin = 2048u; out->relShift = 3u; out->searchSteps = 12u; out->subpix = 192u;
    return 0;
}

int crychic_antialias(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0,
                      uint32_t rows, const crychic_aa_params* params, void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    if (!in_rgba8_dev || !out_rgba8_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 32u * 65535u)) return rc;         // 32 pixel rows per workgroup row
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    crychic_aa_params p;
    crychic_aa_default_params(&p);
    if (params) p = *params;
    if (p.relShift > 31u) return fail(CRYCHIC_E_INVALID_ARG, "anti-aliasing relShift %u outside 0 .. 31", p.relShift);
    if (p.searchSteps == 0 || p.searchSteps > CRYCHIC_AA_MAX_SEARCH)
        return fail(CRYCHIC_E_INVALID_ARG, "anti-aliasing searchSteps %u outside 1 .. %d", p.searchSteps, CRYCHIC_AA_MAX_SEARCH);
    if (p.subpix > 256u) return fail(CRYCHIC_E_INVALID_ARG, "anti-aliasing subpix %u outside 0 .. 256", p.subpix);
    const uintptr_t s = reinterpret_cast<uintptr_t>(in_rgba8_dev), d = reinterpret_cast<uintptr_t>(out_rgba8_dev);
    if ((s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "anti-aliasing planes are not 4-byte aligned");
    const size_t bytes = (size_t)W * H * 4u;
    if (ranges_overlap(s, bytes, d, bytes)) return fail(CRYCHIC_E_INVALID_ARG, "the anti-aliasing input and output planes overlap (the pass cannot run in place)");
    if (int rc = bind(ctx)) return rc;
    const cry::PostAaParams q = { p.absMin, p.relShift, p.searchSteps, p.subpix };
    CRY_HIP(cry::launch_post_aa(in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, q, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_FOG_MAX_STEPS == cry::kFogMaxSteps && sizeof(crychic_fog_params) == 32 && sizeof(crychic_fog_params) == sizeof(cry::FogParams),
              "fog_core.hpp mirrors the ABI");

int crychic_fog_default_params(crychic_fog_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_fog_params{};
    out->density = 0.02f; out->maxDistance = 100.0f; out->steps = 16u;
    out->ambient[0] = 70; out->ambient[1] = 80; out->ambient[2] = 100;
    out->sun[0] = 150; out->sun[1] = 140; out->sun[2] = 110;
    return 0;
}

int crychic_fog(crychic_ctx* ctx, const crychic_pass_constants* cb, const uint32_t* depth_dev, const uint32_t* const shadow_dev[4],
                uint32_t shadowDim, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                const crychic_fog_params* params, void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    if (!cb || !depth_dev || !shadow_dev || !in_rgba8_dev || !out_rgba8_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    uintptr_t align = reinterpret_cast<uintptr_t>(depth_dev) | reinterpret_cast<uintptr_t>(in_rgba8_dev) | reinterpret_cast<uintptr_t>(out_rgba8_dev);
    for (int j = 0; j < 4; ++j) {
        if (!shadow_dev[j]) return fail(CRYCHIC_E_INVALID_ARG, "null argument (cascade map %d)", j);
        align |= reinterpret_cast<uintptr_t>(shadow_dev[j]);
    }
    if (align & 3u) return fail(CRYCHIC_E_INVALID_ARG, "fog planes and maps are not 4-byte aligned");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;                   // a one-dimensional grid, at most 2^27 workgroups
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    if (shadowDim == 0 || shadowDim > CRYCHIC_MAX_SPOT_SHADOW_DIM)
        return fail(CRYCHIC_E_INVALID_ARG, "fog shadowDim %u outside 1 .. %d", shadowDim, CRYCHIC_MAX_SPOT_SHADOW_DIM);
    crychic_fog_params p;
    crychic_fog_default_params(&p);
    if (params) p = *params;
    if (!(p.density >= 0.0f && p.density <= 16.0f)) return fail(CRYCHIC_E_INVALID_ARG, "fog density %g outside 0 .. 16", (double)p.density);
    if (!(p.maxDistance > 0.0f && p.maxDistance <= 3.40282347e38f))
        return fail(CRYCHIC_E_INVALID_ARG, "fog maxDistance %g is not a finite positive number", (double)p.maxDistance);
    if (p.steps == 0 || p.steps > CRYCHIC_FOG_MAX_STEPS) return fail(CRYCHIC_E_INVALID_ARG, "fog steps %u outside 1 .. %d", p.steps, CRYCHIC_FOG_MAX_STEPS);
    if (p.reserved[0] | p.reserved[1] | p.reserved[2]) return fail(CRYCHIC_E_INVALID_ARG, "fog reserved words must be 0");
    // the march takes the shadow coordinates as linear along the ray: exact only for an affine transform
    for (int j = 0; j < 4; ++j) {
        const float* w = cb->ShadowTransforms[j] + 12;
        if (!(w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f && w[3] == 1.0f))
            return fail(CRYCHIC_E_INVALID_ARG, "ShadowTransforms[%d] is not affine (last column %g %g %g %g, not 0 0 0 1)", j, (double)w[0], (double)w[1],
                        (double)w[2], (double)w[3]);
    }
    const uintptr_t s = reinterpret_cast<uintptr_t>(in_rgba8_dev), d = reinterpret_cast<uintptr_t>(out_rgba8_dev);
    const size_t bytes = (size_t)W * H * 4u;
    if (s != d && ranges_overlap(s, bytes, d, bytes))
        return fail(CRYCHIC_E_INVALID_ARG, "the fog input and output planes overlap (in place takes the same address)");
    if (int rc = bind(ctx)) return rc;
    cry::FogParams q;
    std::memcpy(&q, &p, sizeof q);
    CRY_HIP(cry::launch_fog(cb->InvViewProj, cb->EyePosW, cb->ShadowTransforms, depth_dev, shadow_dev, shadowDim, in_rgba8_dev, out_rgba8_dev, W, H,
                            row0, rows, q, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_SSR_MAX_STEPS == cry::kSsrMaxSteps && CRYCHIC_SSR_REFINE == cry::kSsrRefine && sizeof(crychic_ssr_params) == 32 &&
                  sizeof(crychic_ssr_params) == sizeof(cry::SsrParams),
              "ssr_core.hpp mirrors the ABI");

int crychic_ssr_default_params(crychic_ssr_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_ssr_params{};
    out->maxDistance = 20.0f; out->thickness = 0.5f; out->bias = 0.02f; out->maxRoughness = 0.75f;
    out->steps = 32u; out->edgeFade = 32u; out->intensity = 256u;
    return 0;
}

namespace {

// What crychic_ssr and crychic_ssr_glossy check alike, before the context is looked at: a refusal needs no device.  Fills `q` with the
// parameters in force.
int ssr_check(const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev, const float* g2_dev, const uint32_t* depth_dev,
              const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t flags,
              const crychic_ssr_params* params, cry::SsrParams& q)
{
    if (!cb || !g0_dev || !g1_dev || !g2_dev || !depth_dev || !in_rgba8_dev || !out_rgba8_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (flags & ~CRYCHIC_GBUFFER_F16_MASK)
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection flags 0x%x: bits outside CRYCHIC_GBUFFER_G0_F16 | G1_F16 | G2_F16", flags);
    const void* const planes[3] = { g0_dev, g1_dev, g2_dev };
    for (int k = 0; k < 3; ++k) {
        const uintptr_t need = (flags & (CRYCHIC_GBUFFER_G0_F16 << k)) ? 8u : 16u;
        if (reinterpret_cast<uintptr_t>(planes[k]) & (need - 1u))
            return fail(CRYCHIC_E_INVALID_ARG, "G-buffer plane %d is not %u-byte aligned", k, (unsigned)need);
    }
    const uintptr_t s = reinterpret_cast<uintptr_t>(in_rgba8_dev), d = reinterpret_cast<uintptr_t>(out_rgba8_dev);
    if ((reinterpret_cast<uintptr_t>(depth_dev) | s | d) & 3u)
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection depth and frame planes are not 4-byte aligned");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;                   // a one-dimensional grid, at most 2^27 workgroups
    if (W > (1u << 22) || H > (1u << 22)) return fail(CRYCHIC_E_UNSUPPORTED, "frame %ux%u exceeds 2^22 columns or rows", W, H);
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    crychic_ssr_params p;
    crychic_ssr_default_params(&p);
    if (params) p = *params;
    const float big = 3.40282347e38f;
    if (!(p.maxDistance > 0.0f && p.maxDistance <= big))
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection maxDistance %g is not a finite positive number", (double)p.maxDistance);
    if (!(p.thickness > 0.0f && p.thickness <= big))
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection thickness %g is not a finite positive number", (double)p.thickness);
    if (!(p.bias >= 0.0f && p.bias < p.thickness))
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection bias %g outside 0 .. thickness %g", (double)p.bias, (double)p.thickness);
    if (!(p.maxRoughness >= 0.0f && p.maxRoughness <= 1.0f))
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection maxRoughness %g outside 0 .. 1", (double)p.maxRoughness);
    if (p.steps == 0 || p.steps > CRYCHIC_SSR_MAX_STEPS)
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection steps %u outside 1 .. %d", p.steps, CRYCHIC_SSR_MAX_STEPS);
    if (p.edgeFade == 0 || p.edgeFade > 1024u) return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection edgeFade %u outside 1 .. 1024", p.edgeFade);
    if (p.intensity > 256u) return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection intensity %u outside 0 .. 256", p.intensity);
    if (p.reserved) return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection reserved word must be 0");
    const float A = cb->Proj[10], B = cb->Proj[11];
    if (!(A >= -big && A <= big && B >= -big && B <= big) || B == 0.0f)
        return fail(CRYCHIC_E_INVALID_ARG, "Proj[10] = %g and Proj[11] = %g must be finite and Proj[11] not 0 (viewZ = Proj[11] / (d - Proj[10]))",
                    (double)A, (double)B);
    const size_t bytes = (size_t)W * H * 4u;
    if (ranges_overlap(s, bytes, d, bytes))
        return fail(CRYCHIC_E_INVALID_ARG, "the screen-space reflection input and output planes overlap (the pass cannot run in place)");
    std::memcpy(&q, &p, sizeof q);
    return 0;
}

}  // namespace

int crychic_ssr(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev, const float* g2_dev,
                const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                uint32_t flags, const crychic_ssr_params* params, void* stream)
{
    cry::SsrParams q;
    if (int rc = ssr_check(cb, g0_dev, g1_dev, g2_dev, depth_dev, in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, flags, params, q)) return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_ssr(cb->Proj, cb->ViewProj, cb->InvViewProj, cb->EyePosW, cb->NearZ, g0_dev, g1_dev, g2_dev, depth_dev, in_rgba8_dev,
                            out_rgba8_dev, W, H, row0, rows, flags, q, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_SSR_GLOSS_MAX_LEVELS == cry::kSsrGlossMaxLevels && sizeof(crychic_ssr_gloss_params) == 16 &&
                  sizeof(crychic_ssr_gloss_params) == sizeof(cry::SsrGlossParams),
              "ssr_gloss_core.hpp mirrors the ABI");

int crychic_ssr_gloss_default_params(crychic_ssr_gloss_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_ssr_gloss_params{};
    out->coneScale = 0.0f; out->levels = 6u;       // 0: profiles/ssr_gloss_quality.txt
    return 0;
}

size_t crychic_ssr_pyramid_bytes(uint32_t W, uint32_t H, uint32_t levels) { return cry::ssr_pyramid_plan(W, H, levels).bytes; }
size_t crychic_ssr_pyramid_offset(uint32_t W, uint32_t H, uint32_t levels, uint32_t k)
{
    const cry::SsrPyramidPlan plan = cry::ssr_pyramid_plan(W, H, levels);
    return k >= 1u && k <= plan.nEff ? plan.off[k] : 0u;
}

namespace {

// What the two entries check of a pyramid's workspace, the frame's size already checked: `other` is the plane it must not overlap.
int ssr_pyramid_check(uint32_t W, uint32_t H, uint32_t levels, const void* workspace, size_t workspaceBytes, const void* other)
{
    if (levels == 0u || levels > CRYCHIC_SSR_GLOSS_MAX_LEVELS)
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection pyramid levels %u outside 1 .. %d", levels, CRYCHIC_SSR_GLOSS_MAX_LEVELS);
    const size_t need = crychic_ssr_pyramid_bytes(W, H, levels);
    if (need && !workspace) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    const uintptr_t w = reinterpret_cast<uintptr_t>(workspace);
    if (w & 15u) return fail(CRYCHIC_E_INVALID_ARG, "the screen-space reflection pyramid is not 16-byte aligned");
    if (workspaceBytes < need)
        return fail(CRYCHIC_E_INVALID_ARG, "the screen-space reflection pyramid has %zu bytes, %ux%u with %u levels needs %zu", workspaceBytes, W, H, levels, need);
    if (need && ranges_overlap(w, need, reinterpret_cast<uintptr_t>(other), (size_t)W * H * 4u))
        return fail(CRYCHIC_E_INVALID_ARG, "the screen-space reflection pyramid overlaps a plane");
    return 0;
}

}  // namespace

int crychic_ssr_pyramid(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint32_t W, uint32_t H, uint32_t levels, void* workspace_dev, size_t workspace_bytes,
                        void* stream)
{
    if (!in_rgba8_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(in_rgba8_dev) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "the frame plane is not 4-byte aligned");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;                   // one-dimensional grids, at most 2^18 workgroups
    if (int rc = ssr_pyramid_check(W, H, levels, workspace_dev, workspace_bytes, in_rgba8_dev)) return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_ssr_pyramid(in_rgba8_dev, W, H, levels, workspace_dev, (hipStream_t)stream));
    return 0;
}

int crychic_ssr_glossy(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev, const float* g2_dev,
                       const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, const void* pyramid_dev, size_t pyramid_bytes, uint8_t* out_rgba8_dev,
                       uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, uint32_t flags, const crychic_ssr_params* params,
                       const crychic_ssr_gloss_params* gloss, void* stream)
{
    cry::SsrParams q;
    if (int rc = ssr_check(cb, g0_dev, g1_dev, g2_dev, depth_dev, in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, flags, params, q)) return rc;
    crychic_ssr_gloss_params g;
    crychic_ssr_gloss_default_params(&g);
    if (gloss) g = *gloss;
    if (!(g.coneScale >= 0.0f && g.coneScale <= 16.0f))
        return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection coneScale %g outside 0 .. 16", (double)g.coneScale);
    if (g.reserved[0] | g.reserved[1]) return fail(CRYCHIC_E_INVALID_ARG, "screen-space reflection gloss reserved words must be 0");
    if (int rc = ssr_pyramid_check(W, H, g.levels, pyramid_dev, pyramid_bytes, out_rgba8_dev)) return rc;
    if (int rc = bind(ctx)) return rc;
    cry::SsrGlossParams gq;
    std::memcpy(&gq, &g, sizeof gq);
    CRY_HIP(cry::launch_ssr_glossy(cb->Proj, cb->ViewProj, cb->InvViewProj, cb->EyePosW, cb->NearZ, g0_dev, g1_dev, g2_dev, depth_dev, in_rgba8_dev,
                                   pyramid_dev, out_rgba8_dev, W, H, row0, rows, flags, q, gq, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_DOF_MAX_RADIUS == cry::kDofMaxRadius && sizeof(crychic_dof_params) == 32 && sizeof(crychic_dof_params) == sizeof(cry::DofParams),
              "dof_core.hpp mirrors the ABI");

int crychic_dof_default_params(crychic_dof_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_dof_params{};
    out->focusDistance = 15.0f; out->aperture = 6.0f; out->maxRadius = CRYCHIC_DOF_MAX_RADIUS;
    return 0;
}

int crychic_dof(crychic_ctx* ctx, const crychic_pass_constants* cb, const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev,
                uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const crychic_dof_params* params, void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    if (!cb || !depth_dev || !in_rgba8_dev || !out_rgba8_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    const uintptr_t s = reinterpret_cast<uintptr_t>(in_rgba8_dev), d = reinterpret_cast<uintptr_t>(out_rgba8_dev);
    if ((reinterpret_cast<uintptr_t>(depth_dev) | s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "depth-of-field planes are not 4-byte aligned");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;                   // a one-dimensional grid, at most 2^24 workgroups
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    crychic_dof_params p;
    crychic_dof_default_params(&p);
    if (params) p = *params;
    if (!(p.focusDistance > 0.0f && p.focusDistance <= 3.40282347e38f))
        return fail(CRYCHIC_E_INVALID_ARG, "depth-of-field focusDistance %g is not a finite positive number", (double)p.focusDistance);
    if (!(p.aperture >= 0.0f && p.aperture <= 64.0f)) return fail(CRYCHIC_E_INVALID_ARG, "depth-of-field aperture %g outside 0 .. 64", (double)p.aperture);
    if (p.maxRadius == 0 || p.maxRadius > CRYCHIC_DOF_MAX_RADIUS)
        return fail(CRYCHIC_E_INVALID_ARG, "depth-of-field maxRadius %u outside 1 .. %d", p.maxRadius, CRYCHIC_DOF_MAX_RADIUS);
    if (p.reserved[0] | p.reserved[1] | p.reserved[2] | p.reserved[3] | p.reserved[4])
        return fail(CRYCHIC_E_INVALID_ARG, "depth-of-field reserved words must be 0");
    const float A = cb->Proj[10], B = cb->Proj[11];
    const float big = 3.40282347e38f;
    if (!(A >= -big && A <= big && B >= -big && B <= big) || B == 0.0f)
        return fail(CRYCHIC_E_INVALID_ARG, "Proj[10] = %g and Proj[11] = %g must be finite and Proj[11] not 0 (viewZ = Proj[11] / (d - Proj[10]))",
                    (double)A, (double)B);
    const size_t bytes = (size_t)W * H * 4u;
    if (ranges_overlap(s, bytes, d, bytes))
        return fail(CRYCHIC_E_INVALID_ARG, "the depth-of-field input and output planes overlap (the pass cannot run in place)");
    if (int rc = bind(ctx)) return rc;
    cry::DofParams q;
    std::memcpy(&q, &p, sizeof q);
    CRY_HIP(cry::launch_dof(cb->Proj, depth_dev, in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, q, (hipStream_t)stream));
    return 0;
}

static_assert(sizeof(crychic_decal) == 160 && sizeof(cry::DecalTexture) == sizeof(crychic_texture), "crychic_decal is 160 bytes");

int crychic_decal_from_box(const float world[16], uint32_t texW, uint32_t texH, float cosFadeStart, float cosFadeEnd, crychic_decal* out)
{
    if (!world || !out) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(world[k])) return fail(CRYCHIC_E_INVALID_ARG, "decal matrix entry %d is not finite", k);
    if (!(world[12] == 0.0f && world[13] == 0.0f && world[14] == 0.0f && world[15] == 1.0f))
        return fail(CRYCHIC_E_INVALID_ARG, "decal matrix is not affine (last column %g %g %g %g, not 0 0 0 1)", (double)world[12], (double)world[13],
                    (double)world[14], (double)world[15]);
    if (texW == 0 || texH == 0) return fail(CRYCHIC_E_INVALID_ARG, "decal texture size %ux%u must be non-zero", texW, texH);
    if (!(cosFadeStart >= -1.0f && cosFadeStart <= 1.0f && cosFadeEnd >= -1.0f && cosFadeEnd <= 1.0f) || cosFadeStart < cosFadeEnd ||
        (cosFadeStart == cosFadeEnd && cosFadeStart != 1.0f))
        return fail(CRYCHIC_E_INVALID_ARG, "decal fade cosines (%g, %g): both in [-1, 1] and start > end, or (1, 1) for no fade", (double)cosFadeStart,
                    (double)cosFadeEnd);
    // m[r][a]: component r of the cube's axis a; m[r][3]: the centre
    double m[3][4], len[3];
    for (int r = 0; r < 3; ++r)
        for (int a = 0; a < 4; ++a) m[r][a] = (double)world[4 * r + a];
    for (int a = 0; a < 3; ++a) {
        len[a] = std::sqrt(m[0][a] * m[0][a] + m[1][a] * m[1][a] + m[2][a] * m[2][a]);
        if (!(len[a] >= 0x1p-60)) return fail(CRYCHIC_E_INVALID_ARG, "decal matrix is singular (axis %d has length %g)", a, len[a]);
    }
    // the inverse of the 3 x 3 part by cofactors; each axis is scaled to unit length first so that the determinant test is about angles
    double u[3][3];
    for (int r = 0; r < 3; ++r)
        for (int a = 0; a < 3; ++a) u[r][a] = m[r][a] / len[a];
    const double c00 = u[1][1] * u[2][2] - u[1][2] * u[2][1], c01 = u[1][2] * u[2][0] - u[1][0] * u[2][2], c02 = u[1][0] * u[2][1] - u[1][1] * u[2][0];
    const double det = u[0][0] * c00 + u[0][1] * c01 + u[0][2] * c02;
    if (!(std::fabs(det) >= 0x1p-40)) return fail(CRYCHIC_E_INVALID_ARG, "decal matrix is singular (its unit axes span a volume of %g)", det);
    double iu[3][3];        // inverse of u: iu[a][r]
    iu[0][0] = c00 / det; iu[1][0] = c01 / det; iu[2][0] = c02 / det;
    iu[0][1] = (u[0][2] * u[2][1] - u[0][1] * u[2][2]) / det; iu[1][1] = (u[0][0] * u[2][2] - u[0][2] * u[2][0]) / det; iu[2][1] = (u[0][1] * u[2][0] - u[0][0] * u[2][1]) / det;
    iu[0][2] = (u[0][1] * u[1][2] - u[0][2] * u[1][1]) / det; iu[1][2] = (u[0][2] * u[1][0] - u[0][0] * u[1][2]) / det; iu[2][2] = (u[0][0] * u[1][1] - u[0][1] * u[1][0]) / det;
    *out = crychic_decal{};
    for (int a = 0; a < 3; ++a) {
        double t = 0.0;
        for (int r = 0; r < 3; ++r) {
            const double e = iu[a][r] / len[a];
            out->invWorld[4 * a + r] = (float)e;
            t -= e * m[r][3];
        }
        out->invWorld[4 * a + 3] = (float)t;
    }
    for (int r = 0; r < 3; ++r) {
        out->tangentW[r] = (float)u[r][0]; out->bitangentW[r] = (float)u[r][1]; out->normalW[r] = (float)u[r][2];
        out->tint[r] = 1.0f;
    }
    out->opacity = 1.0f;
    const double tx = (double)texW / len[0], ty = (double)texH / len[1];
    out->texelsPerUnit = (float)(tx > ty ? tx : ty);
    if (cosFadeStart == cosFadeEnd) { out->fadeScale = 0.0f; out->fadeBias = 1.0f; }
    else { out->fadeScale = 1.0f / (cosFadeStart - cosFadeEnd); out->fadeBias = -cosFadeEnd * out->fadeScale; }
    double big = 0.0, lo[3], hi[3];
    for (int r = 0; r < 3; ++r) { lo[r] = HUGE_VAL; hi[r] = -HUGE_VAL; }
    for (int k = 0; k < 8; ++k)
        for (int r = 0; r < 3; ++r) {
            const double p = m[r][3] + ((k & 1) ? 0.5 : -0.5) * m[r][0] + ((k & 2) ? 0.5 : -0.5) * m[r][1] + ((k & 4) ? 0.5 : -0.5) * m[r][2];
            lo[r] = p < lo[r] ? p : lo[r]; hi[r] = p > hi[r] ? p : hi[r];
            big = std::fabs(p) > big ? std::fabs(p) : big;
        }
    for (int r = 0; r < 3; ++r) {
        const double pad = 0x1p-10 * ((hi[r] - lo[r]) + big);
        float a = (float)(lo[r] - pad), b = (float)(hi[r] + pad);
        if ((double)a > lo[r] - pad) a = std::nextafterf(a, -HUGE_VALF);
        if ((double)b < hi[r] + pad) b = std::nextafterf(b, HUGE_VALF);
        out->boundsMin[r] = a; out->boundsMax[r] = b;
    }
    out->flags = CRYCHIC_DECAL_ALBEDO;
    out->normalTexture = CRYCHIC_DECAL_NO_TEXTURE;
    return 0;
}

int crychic_apply_decals(crychic_ctx* ctx, const crychic_pass_constants* cb, const uint32_t* depth_dev, void* g0_dev, void* g1_dev, void* g2_dev,
                         uint32_t formatFlags, const crychic_decal* decals_dev, uint32_t nDecals, const crychic_texture* textures,
                         uint32_t nTextures, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    if (!cb || !depth_dev || !g0_dev || !g1_dev || !g2_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (nDecals > 0 && !decals_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument (decals_dev with nDecals %u)", nDecals);
    if (nTextures > 0 && !textures) return fail(CRYCHIC_E_INVALID_ARG, "null argument (textures with nTextures %u)", nTextures);
    if (formatFlags & ~CRYCHIC_GBUFFER_F16_MASK)
        return fail(CRYCHIC_E_INVALID_ARG, "formatFlags 0x%x: bits outside CRYCHIC_GBUFFER_G0_F16 | G1_F16 | G2_F16", formatFlags);
    void* const planes[3] = { g0_dev, g1_dev, g2_dev };
    for (int k = 0; k < 3; ++k) {
        const uintptr_t need = (formatFlags & (CRYCHIC_GBUFFER_G0_F16 << k)) ? 8u : 16u;
        if (reinterpret_cast<uintptr_t>(planes[k]) & (need - 1u))
            return fail(CRYCHIC_E_INVALID_ARG, "G-buffer plane %d is not %u-byte aligned", k, (unsigned)need);
    }
    if ((reinterpret_cast<uintptr_t>(depth_dev) | reinterpret_cast<uintptr_t>(decals_dev)) & 3u)
        return fail(CRYCHIC_E_INVALID_ARG, "the depth plane and the decals are not 4-byte aligned");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;                   // a one-dimensional grid, at most 2^27 workgroups
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    if (nDecals > CRYCHIC_MAX_DECALS) return fail(CRYCHIC_E_INVALID_ARG, "nDecals %u exceeds %d", nDecals, CRYCHIC_MAX_DECALS);
    if (nTextures > CRYCHIC_DECAL_MAX_TEXTURES) return fail(CRYCHIC_E_INVALID_ARG, "nTextures %u exceeds %d", nTextures, CRYCHIC_DECAL_MAX_TEXTURES);
    for (uint32_t k = 0; k < nTextures; ++k) {
        const crychic_texture& t = textures[k];
        if (!t.rgba8_dev || t.width == 0 || t.height == 0)
            return fail(CRYCHIC_E_INVALID_ARG, "decal texture %u: a NULL pointer or a zero side (%ux%u)", k, t.width, t.height);
        if (reinterpret_cast<uintptr_t>(t.rgba8_dev) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "decal texture %u is not 4-byte aligned", k);
        uint32_t most = 0;
        for (uint32_t s = t.width > t.height ? t.width : t.height; s; s >>= 1) ++most;      // floor(log2(max(w, h))) + 1
        if (t.mipLevels > most) return fail(CRYCHIC_E_INVALID_ARG, "decal texture %u: %u levels, a %ux%u texture has at most %u", k, t.mipLevels, t.width, t.height, most);
        if ((uint64_t)t.width * t.height > (1ull << 28)) return fail(CRYCHIC_E_UNSUPPORTED, "decal texture %u: %ux%u exceeds 2^28 texels", k, t.width, t.height);
    }
    for (int k = 8; k < 12; ++k)
        if (!std::isfinite(cb->View[k])) return fail(CRYCHIC_E_INVALID_ARG, "View[%d] = %g is not finite", k, (double)cb->View[k]);
    if (!std::isfinite(cb->Proj[5]) || cb->Proj[5] == 0.0f) return fail(CRYCHIC_E_INVALID_ARG, "Proj[5] = %g must be finite and not 0", (double)cb->Proj[5]);
    if (int rc = bind(ctx)) return rc;
    if (nDecals == 0 || rows == 0) return 0;
    CRY_HIP(cry::launch_decals(cb->View, cb->Proj, depth_dev, g0_dev, g1_dev, g2_dev, formatFlags, decals_dev, nDecals, textures, nTextures, W, H, row0,
                               rows, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_BLOOM_MAX_LEVELS == cry::kBloomMaxLevels && sizeof(crychic_bloom_params) == 32 && sizeof(crychic_bloom_params) == sizeof(cry::BloomParams),
              "bloom_core.hpp mirrors the ABI");

int crychic_bloom_default_params(crychic_bloom_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_bloom_params{};
    out->threshold = 192u; out->knee = 32u; out->scatter = 179u; out->intensity = 128u; out->levels = 6u;
    return 0;
}

size_t crychic_bloom_workspace_bytes(uint32_t W, uint32_t H, uint32_t levels) { return cry::bloom_plan(W, H, levels).bytes; }
size_t crychic_bloom_level_offset(uint32_t W, uint32_t H, uint32_t levels, uint32_t k)
{
    const cry::BloomPlan plan = cry::bloom_plan(W, H, levels);
    return k >= 1u && k <= plan.nEff ? plan.off[k] : 0u;
}

namespace {

// What the three bloom entries check alike, before the context is looked at: `out` is NULL for the pyramid, which has no row range.
// Fills `q` with the parameters in force.
int bloom_check(const uint8_t* in, const uint8_t* out, bool hasOut, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const crychic_bloom_params* params,
                const void* workspace, size_t workspaceBytes, cry::BloomParams& q)
{
    if (!in || (hasOut && !out) || !workspace) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    const uintptr_t s = reinterpret_cast<uintptr_t>(in), d = reinterpret_cast<uintptr_t>(out), w = reinterpret_cast<uintptr_t>(workspace);
    if ((s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "bloom planes are not 4-byte aligned");
    if (w & 15u) return fail(CRYCHIC_E_INVALID_ARG, "the bloom workspace is not 16-byte aligned");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;                   // one-dimensional grids, at most 2^18 workgroups
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    crychic_bloom_params p;
    crychic_bloom_default_params(&p);
    if (params) p = *params;
    if (p.threshold > 255u) return fail(CRYCHIC_E_INVALID_ARG, "bloom threshold %u outside 0 .. 255", p.threshold);
    if (p.knee == 0u || p.knee > 255u) return fail(CRYCHIC_E_INVALID_ARG, "bloom knee %u outside 1 .. 255", p.knee);
    if (p.scatter > 256u) return fail(CRYCHIC_E_INVALID_ARG, "bloom scatter %u outside 0 .. 256", p.scatter);
    if (p.intensity > 1024u) return fail(CRYCHIC_E_INVALID_ARG, "bloom intensity %u outside 0 .. 1024", p.intensity);
    if (p.levels == 0u || p.levels > CRYCHIC_BLOOM_MAX_LEVELS) return fail(CRYCHIC_E_INVALID_ARG, "bloom levels %u outside 1 .. %d", p.levels, CRYCHIC_BLOOM_MAX_LEVELS);
    if (p.reserved[0] | p.reserved[1] | p.reserved[2]) return fail(CRYCHIC_E_INVALID_ARG, "bloom reserved words must be 0");
    const size_t need = crychic_bloom_workspace_bytes(W, H, p.levels);
    if (workspaceBytes < need) return fail(CRYCHIC_E_INVALID_ARG, "the bloom workspace has %zu bytes, %ux%u with %u levels needs %zu", workspaceBytes, W, H, p.levels, need);
    const size_t bytes = (size_t)W * H * 4u;
    if (ranges_overlap(w, need, s, bytes) || (hasOut && ranges_overlap(w, need, d, bytes)))
        return fail(CRYCHIC_E_INVALID_ARG, "the bloom workspace overlaps a plane");
    if (hasOut && s != d && ranges_overlap(s, bytes, d, bytes))
        return fail(CRYCHIC_E_INVALID_ARG, "the bloom input and output planes overlap (in place takes the same address)");
    std::memcpy(&q, &p, sizeof q);
    return 0;
}

}  // namespace

int crychic_bloom_pyramid(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint32_t W, uint32_t H, const crychic_bloom_params* params, void* workspace_dev,
                          size_t workspace_bytes, void* stream)
{
    cry::BloomParams q;
    if (int rc = bloom_check(in_rgba8_dev, nullptr, false, W, H, 0u, 0u, params, workspace_dev, workspace_bytes, q)) return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_bloom_pyramid(in_rgba8_dev, W, H, q, workspace_dev, (hipStream_t)stream));
    return 0;
}

int crychic_bloom_composite(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                            const crychic_bloom_params* params, const void* workspace_dev, size_t workspace_bytes, void* stream)
{
    cry::BloomParams q;
    if (int rc = bloom_check(in_rgba8_dev, out_rgba8_dev, true, W, H, row0, rows, params, workspace_dev, workspace_bytes, q)) return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_bloom_composite(in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, q, workspace_dev, (hipStream_t)stream));
    return 0;
}

int crychic_bloom(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, const crychic_bloom_params* params,
                  void* workspace_dev, size_t workspace_bytes, void* stream)
{
    cry::BloomParams q;
    if (int rc = bloom_check(in_rgba8_dev, out_rgba8_dev, true, W, H, 0u, H, params, workspace_dev, workspace_bytes, q)) return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_bloom_pyramid(in_rgba8_dev, W, H, q, workspace_dev, (hipStream_t)stream));
    CRY_HIP(cry::launch_bloom_composite(in_rgba8_dev, out_rgba8_dev, W, H, 0u, H, q, workspace_dev, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_GRADE_MAX_N == cry::kGradeMaxN && sizeof(crychic_grade_params) == 40 && sizeof(crychic_grade_params) == sizeof(cry::GradeParams),
              "grade_core.hpp mirrors the ABI");
static_assert(4u * CRYCHIC_GRADE_MAX_N * CRYCHIC_GRADE_MAX_N * CRYCHIC_GRADE_MAX_N <= cry::kGradeLdsPerCu, "the largest table fits one compute unit's LDS");

int crychic_grade_default_params(crychic_grade_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    for (int c = 0; c < 3; ++c) { out->slope[c] = 1.0f; out->offset[c] = 0.0f; out->power[c] = 1.0f; }
    out->saturation = 1.0f;
    return 0;
}

namespace {
int check_grade_n(uint32_t N)
{
    if (N < 2u || N > CRYCHIC_GRADE_MAX_N) return fail(CRYCHIC_E_INVALID_ARG, "colour grade table size %u outside 2 .. %d", N, CRYCHIC_GRADE_MAX_N);
    return 0;
}
}  // namespace

int crychic_grade_build_lut(const crychic_grade_params* params, uint32_t N, uint8_t* lut_rgba8, size_t capacityBytes)
{
    if (!lut_rgba8) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (int rc = check_grade_n(N)) return rc;
    if (capacityBytes < (size_t)4u * N * N * N) return fail(CRYCHIC_E_INVALID_ARG, "the colour grade table has %zu bytes, size %u needs %zu", capacityBytes, N, (size_t)4u * N * N * N);
    crychic_grade_params p;
    crychic_grade_default_params(&p);
    if (params) p = *params;
    // !(lo <= v && v <= hi) refuses a NaN with everything else outside the range
    for (int c = 0; c < 3; ++c) {
        if (!(p.slope[c] >= 0.0f && p.slope[c] <= 16.0f)) return fail(CRYCHIC_E_INVALID_ARG, "colour grade slope[%d] %g outside 0 .. 16", c, (double)p.slope[c]);
        if (!(p.offset[c] >= -4.0f && p.offset[c] <= 4.0f)) return fail(CRYCHIC_E_INVALID_ARG, "colour grade offset[%d] %g outside -4 .. 4", c, (double)p.offset[c]);
        if (!(p.power[c] >= 0.0625f && p.power[c] <= 16.0f)) return fail(CRYCHIC_E_INVALID_ARG, "colour grade power[%d] %g outside 1/16 .. 16", c, (double)p.power[c]);
    }
    if (!(p.saturation >= 0.0f && p.saturation <= 4.0f)) return fail(CRYCHIC_E_INVALID_ARG, "colour grade saturation %g outside 0 .. 4", (double)p.saturation);
    cry::GradeParams q;
    memcpy(&q, &p, sizeof q);
    cry::grade_build_lut(q, N, lut_rgba8);
    return 0;
}

int crychic_grade(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                  const uint8_t* lut_rgba8_dev, uint32_t N, void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    if (!in_rgba8_dev || !out_rgba8_dev || !lut_rgba8_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    if (int rc = check_grade_n(N)) return rc;
    const uintptr_t s = reinterpret_cast<uintptr_t>(in_rgba8_dev), d = reinterpret_cast<uintptr_t>(out_rgba8_dev), l = reinterpret_cast<uintptr_t>(lut_rgba8_dev);
    if ((s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "colour grade planes are not 4-byte aligned");
    if (l & 3u) return fail(CRYCHIC_E_INVALID_ARG, "the colour grade table is not 4-byte aligned");
    const size_t bytes = (size_t)W * H * 4u;
    if (s != d && ranges_overlap(s, bytes, d, bytes))
        return fail(CRYCHIC_E_INVALID_ARG, "the colour grade input and output planes overlap (in place takes the same address)");
    if (ranges_overlap(l, (size_t)4u * N * N * N, d, bytes)) return fail(CRYCHIC_E_INVALID_ARG, "the colour grade table overlaps the output plane");
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_grade(in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, lut_rgba8_dev, N, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_SHARPEN_MAX_STRENGTH == cry::kSharpenMaxStrength && CRYCHIC_SHARPEN_MAX_LIMIT == cry::kSharpenMaxLimit &&
              sizeof(crychic_sharpen_params) == 16 && sizeof(crychic_sharpen_params) == sizeof(cry::SharpenParams), "sharpen_core.hpp mirrors the ABI");

int crychic_sharpen_default_params(crychic_sharpen_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    out->strength = CRYCHIC_SHARPEN_DEFAULT_STRENGTH; out->limit = CRYCHIC_SHARPEN_DEFAULT_LIMIT;
    out->reserved[0] = out->reserved[1] = 0u;
    return 0;
}

int crychic_sharpen(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                    const crychic_sharpen_params* params, void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    if (!in_rgba8_dev || !out_rgba8_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    crychic_sharpen_params p;
    crychic_sharpen_default_params(&p);
    if (params) p = *params;
    if (p.strength > CRYCHIC_SHARPEN_MAX_STRENGTH) return fail(CRYCHIC_E_INVALID_ARG, "sharpening strength %u outside 0 .. %d", p.strength, CRYCHIC_SHARPEN_MAX_STRENGTH);
    if (p.limit > CRYCHIC_SHARPEN_MAX_LIMIT) return fail(CRYCHIC_E_INVALID_ARG, "sharpening limit %u outside 0 .. %d", p.limit, CRYCHIC_SHARPEN_MAX_LIMIT);
    if (p.reserved[0] | p.reserved[1]) return fail(CRYCHIC_E_INVALID_ARG, "sharpening reserved words must be 0");
    const uintptr_t s = reinterpret_cast<uintptr_t>(in_rgba8_dev), d = reinterpret_cast<uintptr_t>(out_rgba8_dev);
    if ((s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "sharpening planes are not 4-byte aligned");
    const size_t bytes = (size_t)W * H * 4u;
    if (ranges_overlap(s, bytes, d, bytes)) return fail(CRYCHIC_E_INVALID_ARG, "the sharpening input and output planes overlap (the pass cannot run in place)");
    if (int rc = bind(ctx)) return rc;
    const cry::SharpenParams q = { p.strength, p.limit, { 0u, 0u } };
    CRY_HIP(cry::launch_sharpen(in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, q, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_TAA_RESET == cry::kTaaReset && CRYCHIC_TAA_NO_CLAMP == cry::kTaaNoClamp && sizeof(crychic_taa_params) == 32 &&
              sizeof(crychic_taa_params) == sizeof(cry::TaaParams), "taa_core.hpp mirrors the ABI");

int crychic_taa_default_params(crychic_taa_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_taa_params{};
    out->blend = 26u;
    return 0;
}

size_t crychic_taa_history_bytes(uint32_t W, uint32_t H) { return (size_t)W * H * 8u; }

int crychic_taa(crychic_ctx* ctx, const crychic_pass_constants* cb, const float curViewProj[16], const float prevViewProj[16], const uint32_t* depth_dev,
                const uint8_t* in_rgba8_dev, const uint16_t* history_in_dev, uint16_t* history_out_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H,
                uint32_t row0, uint32_t rows, const crychic_taa_params* params, void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    crychic_taa_params p;
    crychic_taa_default_params(&p);
    if (params) p = *params;
    if (p.blend == 0u || p.blend > 256u) return fail(CRYCHIC_E_INVALID_ARG, "temporal anti-aliasing blend %u outside 1 .. 256", p.blend);
    if (p.flags & ~(CRYCHIC_TAA_RESET | CRYCHIC_TAA_NO_CLAMP)) return fail(CRYCHIC_E_INVALID_ARG, "temporal anti-aliasing flags 0x%x: unknown bits", p.flags);
    for (uint32_t r : p.reserved)
        if (r) return fail(CRYCHIC_E_INVALID_ARG, "temporal anti-aliasing reserved words must be 0");
    const bool reset = (p.flags & CRYCHIC_TAA_RESET) != 0u;
    if (!cb || !curViewProj || !prevViewProj || !depth_dev || !in_rgba8_dev || !history_out_dev || !out_rgba8_dev || (!history_in_dev && !reset))
        return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    const uintptr_t z = reinterpret_cast<uintptr_t>(depth_dev), s = reinterpret_cast<uintptr_t>(in_rgba8_dev), d = reinterpret_cast<uintptr_t>(out_rgba8_dev);
    const uintptr_t hi = reinterpret_cast<uintptr_t>(history_in_dev), ho = reinterpret_cast<uintptr_t>(history_out_dev);
    if ((z | s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "temporal anti-aliasing frame planes are not 4-byte aligned");
    if ((hi | ho) & 7u) return fail(CRYCHIC_E_INVALID_ARG, "temporal anti-aliasing history planes are not 8-byte aligned");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;                   // a one-dimensional grid, at most 2^27 workgroups
    if (W > cry::kTaaMaxSide || H > cry::kTaaMaxSide) return fail(CRYCHIC_E_UNSUPPORTED, "frame %ux%u: temporal anti-aliasing takes at most 2^22 texels a side", W, H);
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(cb->InvViewProj[k]) || !std::isfinite(curViewProj[k]) || !std::isfinite(prevViewProj[k]))
            return fail(CRYCHIC_E_INVALID_ARG, "temporal anti-aliasing: entry %d of InvViewProj, curViewProj or prevViewProj is not finite", k);
    const size_t bytes = (size_t)W * H * 4u, hbytes = crychic_taa_history_bytes(W, H);
    if (ranges_overlap(s, bytes, d, bytes))
        return fail(CRYCHIC_E_INVALID_ARG, "the temporal anti-aliasing input and output planes overlap (the pass reads neighbours: it cannot run in place)");
    if (history_in_dev && ranges_overlap(hi, hbytes, ho, hbytes)) return fail(CRYCHIC_E_INVALID_ARG, "the temporal anti-aliasing history planes overlap");
    for (const uintptr_t h : { hi, ho })
        if (h && (ranges_overlap(h, hbytes, s, bytes) || ranges_overlap(h, hbytes, d, bytes) || ranges_overlap(h, hbytes, z, bytes)))
            return fail(CRYCHIC_E_INVALID_ARG, "a temporal anti-aliasing history plane overlaps a frame plane");
    if (int rc = bind(ctx)) return rc;
    cry::TaaParams q;
    std::memcpy(&q, &p, sizeof q);
    CRY_HIP(cry::launch_taa(cb->InvViewProj, curViewProj, prevViewProj, depth_dev, in_rgba8_dev, reset ? nullptr : history_in_dev, history_out_dev,
                            out_rgba8_dev, W, H, row0, rows, q, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_TAA_UPSCALE_RESET == cry::kTaaReset && CRYCHIC_TAA_UPSCALE_NO_CLAMP == cry::kTaaNoClamp && sizeof(crychic_taa_upscale_params) == 32 &&
              sizeof(crychic_taa_upscale_params) == sizeof(cry::TaaUpscaleParams), "taa_upscale_core.hpp mirrors the ABI");

int crychic_taa_upscale_default_params(crychic_taa_upscale_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_taa_upscale_params{};
    out->blend = 102u;
    return 0;
}

int crychic_taa_upscale(crychic_ctx* ctx, const crychic_pass_constants* cb, const float curViewProj[16], const float prevViewProj[16], float jx, float jy,
                        const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, uint32_t Wi, uint32_t Hi, const uint16_t* history_in_dev,
                        uint16_t* history_out_dev, uint8_t* out_rgba8_dev, uint32_t Wo, uint32_t Ho, uint32_t row0, uint32_t rows,
                        const crychic_taa_upscale_params* params, void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    crychic_taa_upscale_params p;
    crychic_taa_upscale_default_params(&p);
    if (params) p = *params;
    if (p.blend == 0u || p.blend > 256u) return fail(CRYCHIC_E_INVALID_ARG, "temporal upsampling blend %u outside 1 .. 256", p.blend);
    if (p.flags & ~(CRYCHIC_TAA_UPSCALE_RESET | CRYCHIC_TAA_UPSCALE_NO_CLAMP)) return fail(CRYCHIC_E_INVALID_ARG, "temporal upsampling flags 0x%x: unknown bits", p.flags);
    for (uint32_t r : p.reserved)
        if (r) return fail(CRYCHIC_E_INVALID_ARG, "temporal upsampling reserved words must be 0");
    const bool reset = (p.flags & CRYCHIC_TAA_UPSCALE_RESET) != 0u;
    if (!cb || !curViewProj || !prevViewProj || !depth_dev || !in_rgba8_dev || !history_out_dev || !out_rgba8_dev || (!history_in_dev && !reset))
        return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    const uintptr_t z = reinterpret_cast<uintptr_t>(depth_dev), s = reinterpret_cast<uintptr_t>(in_rgba8_dev), d = reinterpret_cast<uintptr_t>(out_rgba8_dev);
    const uintptr_t hi = reinterpret_cast<uintptr_t>(history_in_dev), ho = reinterpret_cast<uintptr_t>(history_out_dev);
    if ((z | s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "temporal upsampling frame planes are not 4-byte aligned");
    if ((hi | ho) & 7u) return fail(CRYCHIC_E_INVALID_ARG, "temporal upsampling history planes are not 8-byte aligned");
    if (Wi == 0 || Hi == 0 || Wo == 0 || Ho == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame sizes %ux%u -> %ux%u must be non-zero", Wi, Hi, Wo, Ho);
    if (Wo < Wi || (uint64_t)Wo > (uint64_t)cry::kTaaUpscaleMaxRatio * Wi || Ho < Hi || (uint64_t)Ho > (uint64_t)cry::kTaaUpscaleMaxRatio * Hi)
        return fail(CRYCHIC_E_INVALID_ARG, "temporal upsampling %ux%u -> %ux%u: each ratio must lie in 1 .. 4", Wi, Hi, Wo, Ho);
    if (int rc = check_extent("output", Wo, Ho, false, 0u)) return rc;                // a one-dimensional grid, at most 2^27 workgroups
    if (Wo > cry::kTaaMaxSide || Ho > cry::kTaaMaxSide) return fail(CRYCHIC_E_UNSUPPORTED, "output %ux%u: temporal upsampling takes at most 2^22 texels a side", Wo, Ho);
    if (int rc = check_rows(kFrameRows, row0, rows, Ho)) return rc;
    if (!std::isfinite(jx) || !std::isfinite(jy) || std::fabs(jx) > 0.5f || std::fabs(jy) > 0.5f)
        return fail(CRYCHIC_E_INVALID_ARG, "temporal upsampling jitter (%g, %g) must be finite and within 0.5 of zero", (double)jx, (double)jy);
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(cb->InvViewProj[k]) || !std::isfinite(curViewProj[k]) || !std::isfinite(prevViewProj[k]))
            return fail(CRYCHIC_E_INVALID_ARG, "temporal upsampling: entry %d of InvViewProj, curViewProj or prevViewProj is not finite", k);
    const size_t ibytes = (size_t)Wi * Hi * 4u, obytes = (size_t)Wo * Ho * 4u, hbytes = crychic_taa_history_bytes(Wo, Ho);
    if (ranges_overlap(s, ibytes, d, obytes) || ranges_overlap(z, ibytes, d, obytes))
        return fail(CRYCHIC_E_INVALID_ARG, "the temporal upsampling output plane overlaps an input plane");
    if (history_in_dev && ranges_overlap(hi, hbytes, ho, hbytes)) return fail(CRYCHIC_E_INVALID_ARG, "the temporal upsampling history planes overlap");
    for (const uintptr_t h : { hi, ho })
        if (h && (ranges_overlap(h, hbytes, s, ibytes) || ranges_overlap(h, hbytes, d, obytes) || ranges_overlap(h, hbytes, z, ibytes)))
            return fail(CRYCHIC_E_INVALID_ARG, "a temporal upsampling history plane overlaps a frame plane");
    if (int rc = bind(ctx)) return rc;
    cry::TaaUpscaleParams q;
    std::memcpy(&q, &p, sizeof q);
    CRY_HIP(cry::launch_taa_upscale(cb->InvViewProj, curViewProj, prevViewProj, jx, jy, depth_dev, in_rgba8_dev, Wi, Hi, reset ? nullptr : history_in_dev,
                                    history_out_dev, out_rgba8_dev, Wo, Ho, row0, rows, q, (hipStream_t)stream));
    return 0;
}

static_assert(sizeof(crychic_motion_blur_params) == 32 && sizeof(crychic_motion_blur_params) == sizeof(cry::MotionBlurParams), "motion_blur_core.hpp mirrors the ABI");

int crychic_motion_blur_default_params(crychic_motion_blur_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_motion_blur_params{};
    out->shutter = 128u; out->samples = 8u; out->maxRadius = 16u;
    return 0;
}

size_t crychic_motion_blur_workspace_bytes(uint32_t W, uint32_t H) { return cry::mb_workspace_bytes(W, H); }
size_t crychic_motion_blur_tile_offset(uint32_t W, uint32_t H) { return cry::mb_tile_offset(W, H); }

namespace {

// What the three motion blur entries check alike, before the context is looked at.  The velocity entry has no frame planes (`frame`
// false: in and out are not looked at), the gather entry no depth plane and no matrices (`reproject` false).  Fills `q` with the
// parameters in force.
int motion_blur_check(bool reproject, bool frame, const crychic_pass_constants* cb, const float* cur, const float* prev, const uint32_t* depth,
                      const uint8_t* in, const uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const crychic_motion_blur_params* params,
                      const void* workspace, size_t workspaceBytes, cry::MotionBlurParams& q)
{
    crychic_motion_blur_params p;
    crychic_motion_blur_default_params(&p);
    if (params) p = *params;
    if (p.shutter > 256u) return fail(CRYCHIC_E_INVALID_ARG, "motion blur shutter %u outside 0 .. 256", p.shutter);
    if (p.samples < 2u || p.samples > 32u || (p.samples & (p.samples - 1u))) return fail(CRYCHIC_E_INVALID_ARG, "motion blur samples %u: not 2, 4, 8, 16 or 32", p.samples);
    if (p.maxRadius == 0u || p.maxRadius > 32u) return fail(CRYCHIC_E_INVALID_ARG, "motion blur maxRadius %u outside 1 .. 32", p.maxRadius);
    if (p.flags) return fail(CRYCHIC_E_INVALID_ARG, "motion blur flags 0x%x: must be 0", p.flags);
    for (uint32_t r : p.reserved)
        if (r) return fail(CRYCHIC_E_INVALID_ARG, "motion blur reserved words must be 0");
    if (!workspace || (reproject && (!cb || !cur || !prev || !depth)) || (frame && (!in || !out))) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    const uintptr_t z = reproject ? reinterpret_cast<uintptr_t>(depth) : 0u, s = frame ? reinterpret_cast<uintptr_t>(in) : 0u;
    const uintptr_t d = frame ? reinterpret_cast<uintptr_t>(out) : 0u, w = reinterpret_cast<uintptr_t>(workspace);
    if ((z | s | d) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "motion blur planes are not 4-byte aligned");
    if (w & 7u) return fail(CRYCHIC_E_INVALID_ARG, "the motion blur workspace is not 8-byte aligned");
    if (W == 0 || H == 0) return fail(CRYCHIC_E_INVALID_ARG, "frame size %ux%u must be non-zero", W, H);
    if (int rc = check_extent("frame", W, H, false, 0u)) return rc;                   // one-dimensional grids, at most 2^20 workgroups
    if (W > cry::kMbMaxSide || H > cry::kMbMaxSide) return fail(CRYCHIC_E_UNSUPPORTED, "frame %ux%u: motion blur takes at most 2^22 texels a side", W, H);
    if (int rc = check_rows(kFrameRows, row0, rows, H)) return rc;
    const size_t need = crychic_motion_blur_workspace_bytes(W, H), bytes = (size_t)W * H * 4u;
    if (workspaceBytes < need) return fail(CRYCHIC_E_INVALID_ARG, "the motion blur workspace has %zu bytes, %ux%u needs %zu", workspaceBytes, W, H, need);
    if (frame && ranges_overlap(s, bytes, d, bytes))
        return fail(CRYCHIC_E_INVALID_ARG, "the motion blur input and output planes overlap (the pass gathers: it cannot run in place)");
    if ((reproject && ranges_overlap(w, need, z, bytes)) || (frame && (ranges_overlap(w, need, s, bytes) || ranges_overlap(w, need, d, bytes))))
        return fail(CRYCHIC_E_INVALID_ARG, "the motion blur workspace overlaps a plane");
    std::memcpy(&q, &p, sizeof q);
    return 0;
}

}  // namespace

int crychic_motion_blur_velocity(crychic_ctx* ctx, const crychic_pass_constants* cb, const float curViewProj[16], const float prevViewProj[16],
                                 const uint32_t* depth_dev, uint32_t W, uint32_t H, const crychic_motion_blur_params* params, void* workspace_dev,
                                 size_t workspace_bytes, void* stream)
{
    cry::MotionBlurParams q;
    if (int rc = motion_blur_check(true, false, cb, curViewProj, prevViewProj, depth_dev, nullptr, nullptr, W, H, 0u, H, params, workspace_dev, workspace_bytes, q))
        return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_motion_blur_velocity(cb->InvViewProj, curViewProj, prevViewProj, depth_dev, W, H, q, workspace_dev, (hipStream_t)stream));
    return 0;
}

int crychic_motion_blur_gather(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                               const crychic_motion_blur_params* params, const void* workspace_dev, size_t workspace_bytes, void* stream)
{
    cry::MotionBlurParams q;
    if (int rc = motion_blur_check(false, true, nullptr, nullptr, nullptr, nullptr, in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, params, workspace_dev,
                                   workspace_bytes, q))
        return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_motion_blur_gather(in_rgba8_dev, out_rgba8_dev, W, H, row0, rows, q, workspace_dev, (hipStream_t)stream));
    return 0;
}

int crychic_motion_blur(crychic_ctx* ctx, const crychic_pass_constants* cb, const float curViewProj[16], const float prevViewProj[16], const uint32_t* depth_dev,
                        const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, const crychic_motion_blur_params* params,
                        void* workspace_dev, size_t workspace_bytes, void* stream)
{
    cry::MotionBlurParams q;
    if (int rc = motion_blur_check(true, true, cb, curViewProj, prevViewProj, depth_dev, in_rgba8_dev, out_rgba8_dev, W, H, 0u, H, params, workspace_dev,
                                   workspace_bytes, q))
        return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_motion_blur_velocity(cb->InvViewProj, curViewProj, prevViewProj, depth_dev, W, H, q, workspace_dev, (hipStream_t)stream));
    CRY_HIP(cry::launch_motion_blur_gather(in_rgba8_dev, out_rgba8_dev, W, H, 0u, H, q, workspace_dev, (hipStream_t)stream));
    return 0;
}

size_t crychic_cube_sh_offset(uint32_t dim, uint32_t levels) { return cry::ambient_sh_offset(dim, levels); }
size_t crychic_cube_chain_sh_bytes(uint32_t dim, uint32_t levels) { return cry::ambient_sh_offset(dim, levels) + CRYCHIC_CUBE_SH_BYTES; }

int crychic_project_cube_sh(crychic_ctx* ctx, const uint8_t* level_dev, uint32_t d, void* tail_dev, void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (!level_dev || !tail_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (d == 0 || d > 8192u) return fail(CRYCHIC_E_INVALID_ARG, "cube map face size %u outside 1 .. 8192", d);
    const uintptr_t s = reinterpret_cast<uintptr_t>(level_dev), t = reinterpret_cast<uintptr_t>(tail_dev);
    if (s & 3u) return fail(CRYCHIC_E_INVALID_ARG, "cube map level is not 4-byte aligned");
    if (t & 7u) return fail(CRYCHIC_E_INVALID_ARG, "environment tail is not 8-byte aligned");
    const size_t bytes = (size_t)6u * d * d * 4u;
    if (ranges_overlap(s, bytes, t, CRYCHIC_CUBE_SH_BYTES)) return fail(CRYCHIC_E_INVALID_ARG, "the environment tail overlaps the level");
    CRY_HIP(cry::launch_cube_sh(level_dev, d, tail_dev, (hipStream_t)stream));
    return 0;
}

size_t crychic_cube_env_brdf_offset(uint32_t dim, uint32_t levels) { return cry::env_brdf_offset(dim, levels); }
size_t crychic_cube_chain_env_bytes(uint32_t dim, uint32_t levels) { return cry::env_brdf_offset(dim, levels) + CRYCHIC_ENV_BRDF_BYTES; }

int crychic_build_env_brdf(crychic_ctx* ctx, void* table_dev, void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (!table_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(table_dev) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "environment BRDF table is not 4-byte aligned");
    CRY_HIP(cry::launch_env_brdf(table_dev, (hipStream_t)stream));
    return 0;
}

size_t crychic_cube_probe_offset(uint32_t dim, uint32_t levels) { return cry::parallax_probe_offset(dim, levels); }

int crychic_set_cube_probe_volume(crychic_ctx* ctx, void* tail_dev, const float pos[3], const float boxMin[3], const float boxMax[3],
                                  void* stream)
{
    if (int rc = bind(ctx)) return rc;
    if (!tail_dev || !pos || !boxMin || !boxMax) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(tail_dev) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "environment tail is not 4-byte aligned");
    if (!cry::probe_volume_valid(pos, boxMin, boxMax))
        return fail(CRYCHIC_E_INVALID_ARG, "probe volume: every value finite and boxMin < pos < boxMax in every component");
    CRY_HIP(cry::launch_cube_probe_volume(tail_dev, pos, boxMin, boxMax, (hipStream_t)stream));
    return 0;
}

static_assert(CRYCHIC_SKY_MAX_VIEW_STEPS == cry::kSkyMaxViewSteps && CRYCHIC_SKY_MAX_SUN_STEPS == cry::kSkyMaxSunSteps &&
                  sizeof(crychic_sky_params) == 48 && sizeof(crychic_sky_params) == sizeof(cry::SkyParams),
              "sky_core.hpp mirrors the ABI");

int crychic_sky_default_params(crychic_sky_params* out)
{
    if (!out) return fail(CRYCHIC_E_INVALID_ARG, "out is null");
    *out = crychic_sky_params{};
    out->sunDir[0] = 0.0f; out->sunDir[1] = 0.5f; out->sunDir[2] = -0.8660254f;      // 30 degrees up
    out->altitude = 0.002f; out->sunIntensity = 20.0f; out->exposure = 2.0f;
    out->sunAngularRadius = 0.02f; out->groundAlbedo = 0.3f;
    out->viewSteps = 16u; out->sunSteps = 8u;
    return 0;
}

namespace {
// The parameters of a sky call, with the defaults for NULL; a refusal leaves the message behind.
int sky_params(const crychic_sky_params* params, cry::SkyParams* q)
{
    crychic_sky_params p;
    crychic_sky_default_params(&p);
    if (params) p = *params;
    const auto in = [](float v, float lo, float hi) { return v >= lo && v <= hi; };       // false for NaN
    for (int c = 0; c < 3; ++c)
        if (!in(p.sunDir[c], -3.40282347e38f, 3.40282347e38f)) return fail(CRYCHIC_E_INVALID_ARG, "sky sunDir[%d] %g is not finite", c, (double)p.sunDir[c]);
    if (p.sunDir[0] == 0.0f && p.sunDir[1] == 0.0f && p.sunDir[2] == 0.0f) return fail(CRYCHIC_E_INVALID_ARG, "sky sunDir is the zero vector");
    if (!in(p.altitude, 0.0f, 50.0f)) return fail(CRYCHIC_E_INVALID_ARG, "sky altitude %g outside 0 .. 50 km", (double)p.altitude);
    if (!in(p.sunIntensity, 0.0f, 65536.0f)) return fail(CRYCHIC_E_INVALID_ARG, "sky sunIntensity %g outside 0 .. 65536", (double)p.sunIntensity);
    if (!in(p.exposure, 0.0f, 65536.0f)) return fail(CRYCHIC_E_INVALID_ARG, "sky exposure %g outside 0 .. 65536", (double)p.exposure);
    if (!in(p.sunAngularRadius, 0.0f, 0.5f)) return fail(CRYCHIC_E_INVALID_ARG, "sky sunAngularRadius %g outside 0 .. 0.5", (double)p.sunAngularRadius);
    if (!in(p.groundAlbedo, 0.0f, 1.0f)) return fail(CRYCHIC_E_INVALID_ARG, "sky groundAlbedo %g outside 0 .. 1", (double)p.groundAlbedo);
    if (p.viewSteps == 0 || p.viewSteps > CRYCHIC_SKY_MAX_VIEW_STEPS)
        return fail(CRYCHIC_E_INVALID_ARG, "sky viewSteps %u outside 1 .. %d", p.viewSteps, CRYCHIC_SKY_MAX_VIEW_STEPS);
    if (p.sunSteps == 0 || p.sunSteps > CRYCHIC_SKY_MAX_SUN_STEPS)
        return fail(CRYCHIC_E_INVALID_ARG, "sky sunSteps %u outside 1 .. %d", p.sunSteps, CRYCHIC_SKY_MAX_SUN_STEPS);
    if (p.reserved[0] | p.reserved[1]) return fail(CRYCHIC_E_INVALID_ARG, "sky reserved words must be 0");
    std::memcpy(q, &p, sizeof *q);
    return 0;
}
}  // namespace

int crychic_render_sky(crychic_ctx* ctx, uint8_t* cube_dev, uint32_t dim, uint32_t face0, uint32_t faces, const crychic_sky_params* params,
                       void* stream)
{
    // every argument is checked before the context is looked at: a refusal needs no device
    if (!cube_dev) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(cube_dev) & 3u) return fail(CRYCHIC_E_INVALID_ARG, "cube map is not 4-byte aligned");
    if (dim < 2u || dim > 8192u) return fail(CRYCHIC_E_INVALID_ARG, "cube map face size %u outside 2 .. 8192", dim);
    if (face0 > 6u || faces > 6u - face0) return fail(CRYCHIC_E_INVALID_ARG, "faces [%u,+%u) outside the six faces", face0, faces);
    cry::SkyParams q;
    if (int rc = sky_params(params, &q)) return rc;
    if (int rc = bind(ctx)) return rc;
    CRY_HIP(cry::launch_sky(cube_dev, dim, face0, faces, q, (hipStream_t)stream));
    return 0;
}

int crychic_sky_sun_colour(const crychic_sky_params* params, float rgb[3])
{
    if (!rgb) return fail(CRYCHIC_E_INVALID_ARG, "null argument");
    cry::SkyParams q;
    if (int rc = sky_params(params, &q)) return rc;
    cry::sky_sun_colour(q, rgb);
    return 0;
}

int crychic_strip_rows(uint32_t H, int nranks, int rank, uint32_t* row0, uint32_t* rows)
{
    if (!row0 || !rows || nranks <= 0 || rank < 0 || rank >= nranks || (H & 1u))
        return fail(CRYCHIC_E_INVALID_ARG, "bad strip request (H=%u nranks=%d rank=%d)", H, nranks, rank);
    const uint32_t pairs = H / 2;                    // strips are whole half-res rows
    const uint32_t per = pairs / (uint32_t)nranks;   // last rank takes the remainder
    const uint32_t p0 = per * (uint32_t)rank;
    const uint32_t p1 = (rank == nranks - 1) ? pairs : p0 + per;
    *row0 = 2 * p0;
    *rows = 2 * (p1 - p0);
    return 0;
}

}  // extern "C"
