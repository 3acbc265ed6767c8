// Host build of the per-lane predicates behind the wave votes of the lighting kernels (csrc/light_core.hpp, csrc/light_tiles.hpp),
// for tests/light_votes_lib.py: for one lighting call it says of every pixel of the row range what that pixel's lane would answer
// in each vote, so that a test can sort the wavefronts of the call on the CPU -- unanimous, refused by exactly one lane, mixed --
// and assert that its frames make the device take every shortcut and every general path.  A predicate that is a product function,
// or a function of what one returns, is computed with that function; one that is a local expression of a kernel body is restated
// here, next to the line it copies.  TEST HARNESS ONLY.
#include <cstdint>
#include "light_core.hpp"
#include "light_bind.hpp"

using namespace cry;

namespace {

enum Field : uint32_t {
    F_COVERED = 0,      // depth below the clear value (light_tiles.hpp:110,135)
    F_J,                // cascade_index(distance)
    F_BLEND,            // the pixel blends cascades j and j + 1 (light_core.hpp:1014)
    F_NEEDS,            // bit k: the pixel needs cascade k (mine | next, :1021)
    F_P10,              // J <= 2 and |posW| < 1e15 (:1074 without `j == J`, which the grouping adds: J is the first lane's)
    F_P11,              // both footprints inside their maps (cascade_uniform_fetch's c.inside on the host)
    F_P12,              // both factors 0 or 1 (:1154)
    F_P1A, F_P1B,       // all four texels of the footprint of cascade j / j + 1 inside the map (:85-88)
    F_P2,               // four fields: the tap of cascade k is 0 or 1 (:118)
    F_P3 = F_P2 + 4,    // four fields: pcf_taps_inside of cascade k
    F_P8 = F_P3 + 4,    // shadowWIsOne and |posW| < 1.2676506e30 (:997)
    F_P4,               // the cube lookup's footprint inside its face (:461); of a sky pixel: the lookup along its view ray
    F_P5,               // lod == 0 (cube_chain_flat); of a sky pixel: sky_pixel_chain's lod
    F_P6,               // the projected footprint inside the half-res map (:790)
    F_P7,               // all four ambient texels 65535 (:827)
    F_COUNT
};

// light_core.hpp:190-191 under :1003-1011: the lookup coordinates of cascade k, W_ONE form when the lane's own wOne holds (x / 1 == x:
// the same bits either way for such a lane, whichever instantiation its wavefront runs)
struct Lookup { float x, y, depth; };
Lookup cascade_lookup(const LightParams& P, f3 posW, int k, bool wOne)
{
    const float* T = P.ShadowTransforms[k];
    const float spx = mulcol1(posW.x, posW.y, posW.z, T + 0), spy = mulcol1(posW.x, posW.y, posW.z, T + 4);
    const float spz = mulcol1(posW.x, posW.y, posW.z, T + 8);
    if (wOne) return Lookup{ spx, spy, spz };
    const float rw = rcp(mulcol1(posW.x, posW.y, posW.z, T + 12));
    return Lookup{ spx * rw, spy * rw, spz * rw };
}

// light_core.hpp:441-461: cube_address's `inside`
bool cube_footprint_inside(uint32_t dim, f3 r)
{
    const float ax = __builtin_fabsf(r.x), ay = __builtin_fabsf(r.y), az = __builtin_fabsf(r.z);
    const bool isx = (ax >= ay) & (ax >= az), isy = !isx & (ay >= az);
    const bool px = r.x >= 0.0f, py = r.y >= 0.0f, pz = r.z >= 0.0f;
    const float ma = isx ? ax : (isy ? ay : az);
    const float sc = isx ? (px ? -r.z : r.z) : (isy ? r.x : (pz ? r.x : -r.x));
    const float tc = isx ? -r.y : (isy ? (py ? r.z : -r.z) : -r.y);
    const float rma = rcp(ma);
    const float u = fma(0.5f, sc * rma, 0.5f), v = fma(0.5f, tc * rma, 0.5f);
    const float fd = (float)dim;
    const float tx = fma(u, fd, -0.5f), ty = fma(v, fd, -0.5f);
    const float flx = __builtin_floorf(tx), fly = __builtin_floorf(ty);
    return (flx >= 0.0f) & (flx <= fd - 2.0f) & (fly >= 0.0f) & (fly <= fd - 2.0f);
}

// light_core.hpp:777-790: ambient_fetch_projected's `inside` for a frame with an ambient map (W >= 4)
bool ambient_footprint_inside(const LightParams& P, f3 posW)
{
    const v2f c0{ P.ScreenPairs[0][0], P.ScreenPairs[0][1] }, c1{ P.ScreenPairs[1][0], P.ScreenPairs[1][1] };
    const v2f c2{ P.ScreenPairs[2][0], P.ScreenPairs[2][1] }, c3{ P.ScreenPairs[3][0], P.ScreenPairs[3][1] };
    const v2f s = fma2(splat(posW.z), c2, fma2(splat(posW.y), c1, splat(posW.x) * c0)) + c3;
    const float rsw = rcp(mulcol1(posW.x, posW.y, posW.z, P.ViewProjTex + 12));
    const v2f uv = s * rsw;
    const v2f dims{ P.halfDims[0], P.halfDims[1] };
    const v2f t = fma2(uv, dims, -0.5f);
    const v2f fl = floor2(t);
    return (fl.x >= 0.0f) & (fl.x <= dims.x - 2.0f) & (fl.y >= 0.0f) & (fl.y <= dims.y - 2.0f);
}

bool zero_or_one(float t) { return (t == 0.0f) | (t == 1.0f); }

}  // namespace

extern "C" {

uint32_t lv_field_count(void) { return F_COUNT; }

// The fields of every pixel of rows [row0, row0 + rows) of one crychic_deferred_light call over float4 planes, out[(y * W + x) *
// lv_field_count() + field]; a pixel outside the rows keeps what out held.  Every field is computed for every pixel, covered or not
// (what an uncovered lane WOULD answer shows that it does not vote); fields of lookups the pixel's own values rule out are 0.
// ambient must not be null, W >= 4.  The derivative chain (CRYCHIC_LIGHT_CUBE_LEVELS > 1 without gloss) takes its level of detail from the quad.
void lv_classify(const crychic_pass_constants* cb, const float* g0, const float* g2, const uint32_t* depth, const uint16_t* ambient,
                 const uint32_t* const shadow[4], uint32_t shadowDim, const uint8_t* cube, uint32_t cubeDim, uint32_t W, uint32_t H,
                 uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags, uint8_t* out)
{
    LightParams P;
    bind_light_params(P, *cb, shadow, shadowDim, cubeDim, W, H, numDirLights, pcfSearchRadius, flags);
    const bool fixQ1 = (flags & CRYCHIC_FIX_Q1) != 0;
    const bool chain = P.cubeLevels > 1u && !(flags & CRYCHIC_LIGHT_CUBE_GLOSS);      // light_variant's derivative chain
    const uint32_t row1 = row0 + rows;
    auto shaded = [&](uint32_t x, uint32_t y) { return x < W && y < row1 && (depth[y * W + x] & 0x00FFFFFFu) < 0x00FFFFFFu; };
    auto G = [&](const float* g, uint32_t idx) { return f4a{ g[4 * idx], g[4 * idx + 1], g[4 * idx + 2], g[4 * idx + 3] }; };
    auto reflection = [&](uint32_t x, uint32_t y) { return reflection_dir(P, G(g0, y * W + x), G(g2, y * W + x)); };
    for (uint32_t y = row0; y < row1; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t idx = y * W + x;
            uint8_t* o = out + (size_t)idx * F_COUNT;
            for (uint32_t k = 0; k < F_COUNT; ++k) o[k] = 0;
            const bool covered = (depth[idx] & 0x00FFFFFFu) < 0x00FFFFFFu;
            o[F_COVERED] = covered;
            const f4a G0 = G(g0, idx), G2 = G(g2, idx);
            const f3 posW{ G0.x, G0.y, G0.z };
            // light_pixel :1272-1275
            const f3 toEye{ P.EyePosW[0] - posW.x, P.EyePosW[1] - posW.y, P.EyePosW[2] - posW.z };
            const float distance = len_from_sq(dot3(toEye, toEye));
            const int j = cascade_index(distance);
            o[F_J] = (uint8_t)j;
            const float radiusJ = j == 0 ? 30.0f : (j == 1 ? 50.0f : (j == 2 ? 80.0f : 100.0f));           // :1013-1014
            const bool blend = j < 3 && (!fixQ1 || __builtin_fabsf(distance - radiusJ) < 5.0f);
            o[F_BLEND] = blend;
            const float pmax = 1.2676506e30f;                                                               // :996-997
            const bool wOne = P.shadowWIsOne && __builtin_fabsf(posW.x) < pmax && __builtin_fabsf(posW.y) < pmax && __builtin_fabsf(posW.z) < pmax;
            o[F_P8] = wOne;
            const bool small = __builtin_fabsf(posW.x) < 1.0e15f && __builtin_fabsf(posW.y) < 1.0e15f && __builtin_fabsf(posW.z) < 1.0e15f;   // :1068,1074
            o[F_P10] = j <= 2 && small;
            for (int k = 0; k < 4 && j < 4; ++k) {
                const bool mine = j == k, next = blend & (j + 1 == k);                                      // :1021
                if (!(mine | next)) continue;
                o[F_NEEDS] |= (uint8_t)(1u << k);
                const Lookup l = cascade_lookup(P, posW, k, wOne);
                o[F_P2 + k] = zero_or_one(shadow_cmp_linear(P.shadow[k], P.shadowDim, l.x, l.y, l.depth));
                o[F_P3 + k] = pcf_taps_inside(P.shadowDim, l.x, l.y, l.depth, pcfSearchRadius);
            }
            if (o[F_P10] && P.shadowWIsOne) {        // what the packed path would see of this lane (it takes only such lanes)
                CascadeTexels c;
                cascade_uniform_fetch(P, posW, j, c);
                o[F_P11] = c.inside;
                const uint32_t dim = P.shadowDim;
                o[F_P1A] = c.inside || ((uint32_t)c.ia < dim && (uint32_t)(c.ia + 1) < dim && (uint32_t)c.ja < dim && (uint32_t)(c.ja + 1) < dim);   // :85-86
                o[F_P1B] = c.inside || ((uint32_t)c.ib < dim && (uint32_t)(c.ib + 1) < dim && (uint32_t)c.jb < dim && (uint32_t)(c.jb + 1) < dim);
                const Lookup a = cascade_lookup(P, posW, j, true), b = cascade_lookup(P, posW, j + 1, true);
                o[F_P12] = zero_or_one(shadow_cmp_linear(P.shadow[j], dim, a.x, a.y, a.depth)) &&
                           zero_or_one(shadow_cmp_linear(P.shadow[j + 1], dim, b.x, b.y, b.depth));
            }
            o[F_P6] = ambient_footprint_inside(P, posW);
            const AmbientPairs af = ambient_fetch_projected(P, ambient, true, (const uint16_t*)cube, posW);
            o[F_P7] = (af.d0 & af.d1) == 0xFFFFFFFFu;
            if (covered || !(flags & CRYCHIC_LIGHT_SKY)) {
                const f3 r = reflection_dir(P, G0, G2);
                o[F_P4] = cube_footprint_inside(cubeDim, r);
                float lod = 0.0f;
                if (chain) {        // host_light.hpp's restatement of quad_reflection_lod: neighbours the pass shades
                    f3 ddx{ 0.0f, 0.0f, 0.0f }, ddy{ 0.0f, 0.0f, 0.0f };
                    if (shaded(x ^ 1u, y)) { const f3 n = reflection(x ^ 1u, y); ddx = (x & 1u) ? f3{ r.x - n.x, r.y - n.y, r.z - n.z } : f3{ n.x - r.x, n.y - r.y, n.z - r.z }; }
                    if (shaded(x, y ^ 1u)) { const f3 n = reflection(x, y ^ 1u); ddy = (y & 1u) ? f3{ r.x - n.x, r.y - n.y, r.z - n.z } : f3{ n.x - r.x, n.y - r.y, n.z - r.z }; }
                    lod = cube_lod(P.cubeDim, P.cubeLevels, r, ddx, ddy);
                }
                o[F_P5] = lod == 0.0f;
            } else {
                const f3 d = sky_direction(P, x, y);
                o[F_P4] = cube_footprint_inside(cubeDim, d);
                float lod = 0.0f;
                if (chain) {        // light_core.hpp:1378-1382
                    f3 ddx{ 0.0f, 0.0f, 0.0f }, ddy{ 0.0f, 0.0f, 0.0f };
                    if ((x ^ 1u) < P.W) { const f3 n = sky_direction(P, x ^ 1u, y); ddx = (x & 1u) ? f3{ d.x - n.x, d.y - n.y, d.z - n.z } : f3{ n.x - d.x, n.y - d.y, n.z - d.z }; }
                    if ((y ^ 1u) < P.H) { const f3 n = sky_direction(P, x, y ^ 1u); ddy = (y & 1u) ? f3{ d.x - n.x, d.y - n.y, d.z - n.z } : f3{ n.x - d.x, n.y - d.y, n.z - d.z }; }
                    lod = cube_lod(P.cubeDim, P.cubeLevels, d, ddx, ddy);
                }
                o[F_P5] = lod == 0.0f;
            }
        }
}

}
