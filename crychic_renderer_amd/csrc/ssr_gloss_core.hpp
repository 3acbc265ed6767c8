// ssr_gloss_core.hpp -- the body of crychic_ssr_glossy (include/crychic_hip.h states the definition), built for
// the device (ssr_gloss.hip) and for the host (tests/ssr_gloss_host).  The pass is ssr_pixel (ssr_core.hpp) with another policy for
// the hit colour: steps 6a and 6b, the level of the frame's pyramid whose texel is as wide as the reflection cone at the hit, fetched
// bilinearly and blended with the next level, all in integers behind the level itself.
//
// The kernel's shape, behind ssr_pixel's own votes:
//   * a wavefront none of whose lanes has lq > 0 (mirrors, short rays, coneScale 0, one level) takes the point sample, as crychic_ssr
//     does: the general fetch at lq == 0 is that texel exactly;
//   * level k + 1 is fetched only if some lane has f > 0;
//   * a lane's level is its own, so its sizes come from shifts of W and H and its offset from a chain of selects over the kernel's
//     arguments: no table is indexed by a lane's value;
//   * lam lies in [0, n_eff] before it is converted to an integer.
#pragma once
#include "ssr_core.hpp"
#include "ssr_pyramid_core.hpp"

namespace cry {

struct SsrGlossParams { float coneScale; uint32_t levels, reserved[2]; };       // crychic_ssr_gloss_params

struct SsrGlossArgs {
    SsrArgs s;
    const uint32_t* pyr;                        // the workspace of crychic_ssr_pyramid; never read when nEff == 0
    uint32_t off[kSsrGlossMaxLevels];           // level k's first texel, in texels (off[0] unused)
    uint32_t nEff;
    float coneScale, nEffF;
};

struct SsrGlossLaunch { SsrGlossArgs args; uint32_t groups; };

inline SsrGlossLaunch ssr_gloss_launch(const SsrLaunch& base, const void* pyramid, const SsrGlossParams& g)
{
    SsrGlossLaunch L;
    L.args.s = base.args;
    L.groups = base.groups;
    const SsrPyramidPlan plan = ssr_pyramid_plan(base.args.W, base.args.H, g.levels);
    L.args.pyr = static_cast<const uint32_t*>(pyramid);
    for (uint32_t k = 0; k < kSsrGlossMaxLevels; ++k) L.args.off[k] = (uint32_t)(plan.off[k] >> 2);        // below 2^28 texels in all
    L.args.nEff = plan.nEff;
    L.args.nEffF = (float)plan.nEff;
    L.args.coneScale = g.coneScale;
    return L;
}

// fetch(k) of step 6b at hit pixel (hx, hy): R | B << 16 and G in 0 .. 255 each.  k <= nEff: every index is a clamped coordinate pair
// of level k, below W_k H_k texels from the level's start.
struct SsrGlossTexel { uint32_t rb, g; };
CRY_HD SsrGlossTexel ssr_gloss_fetch(const SsrGlossArgs& a, uint32_t k, uint32_t hx, uint32_t hy)
{
    const uint32_t wk = (a.s.W + (1u << k) - 1u) >> k, hk = (a.s.H + (1u << k) - 1u) >> k;      // W_k = ceil(W / 2^k)
    uint32_t off = 0u;
#pragma unroll
    for (uint32_t j = 1; j < kSsrGlossMaxLevels; ++j) off = k == j ? a.off[j] : off;
    const uint32_t* base = k == 0u ? a.s.in : a.pyr;
    const uint32_t Tx = ((2u * hx + 1u) * 128u) >> k, Ty = ((2u * hy + 1u) * 128u) >> k;       // hx, hy below 2^22
    const uint32_t Ux = (Tx > 128u ? Tx : 128u) - 128u, Uy = (Ty > 128u ? Ty : 128u) - 128u;
    const uint32_t x0 = (Ux >> 8) < wk - 1u ? (Ux >> 8) : wk - 1u, x1 = x0 + 1u < wk - 1u ? x0 + 1u : wk - 1u, fx = Ux & 255u;
    const uint32_t y0 = (Uy >> 8) < hk - 1u ? (Uy >> 8) : hk - 1u, y1 = y0 + 1u < hk - 1u ? y0 + 1u : hk - 1u, fy = Uy & 255u;
    const uint32_t r0 = off + y0 * wk, r1 = off + y1 * wk;
    const uint32_t c00 = base[r0 + x0], c10 = base[r0 + x1], c01 = base[r1 + x0], c11 = base[r1 + x1];
    // along x two channels to a dword: a half holds at most 255 * 256
    const uint32_t gx = 256u - fx, gy = 256u - fy;
    const uint32_t topRB = (c00 & kSsrPyrMask) * gx + (c10 & kSsrPyrMask) * fx, botRB = (c01 & kSsrPyrMask) * gx + (c11 & kSsrPyrMask) * fx;
    const uint32_t topG = ((c00 >> 8) & 255u) * gx + ((c10 >> 8) & 255u) * fx, botG = ((c01 >> 8) & 255u) * gx + ((c11 >> 8) & 255u) * fx;
    const uint32_t R = ((topRB & 0xFFFFu) * gy + (botRB & 0xFFFFu) * fy + 32768u) >> 16;
    const uint32_t B = ((topRB >> 16) * gy + (botRB >> 16) * fy + 32768u) >> 16;
    const uint32_t G = (topG * gy + botG * fy + 32768u) >> 16;
    return SsrGlossTexel{ R | (B << 16), G };
}

// crychic_ssr_glossy's policy for ssr_pixel's hit colour: steps 6a and 6b.
struct SsrGlossHit {
    const SsrGlossArgs& g;
    template <class Any>
    CRY_HD uint32_t operator()(const SsrArgs& a, uint32_t px, uint32_t py, uint32_t hitIdx, float rough, bool hit, Any any) const
    {
        const uint32_t hy = hitIdx / a.W, hx = hitIdx - hy * a.W;
        // 6a
        const float dx = (float)hx - (float)px, dy = (float)hy - (float)py;
        const float Lpx = len_from_sq(fma(dx, dx, dy * dy));
        const float r = (g.coneScale * rough) * Lpx;
        float lam = r > 1.0f ? det_log2(r) : 0.0f;             // a NaN gives 0; r > 1: lam >= 0
        lam = lam < g.nEffF ? lam : g.nEffF;
        const uint32_t lq = hit ? (uint32_t)fma(lam, 256.0f, 0.5f) : 0u;        // lam in [0, nEff]: 0 .. 256 nEff
        if (!any(lq > 0u)) return a.in[hitIdx];
        // 6b
        const uint32_t k = lq >> 8, f = lq & 255u;              // k == nEff has f == 0
        SsrGlossTexel v = ssr_gloss_fetch(g, k, hx, hy);
        if (any(f > 0u)) {
            const SsrGlossTexel u = ssr_gloss_fetch(g, f > 0u ? k + 1u : k, hx, hy);
            v.rb = ((v.rb * (256u - f) + u.rb * f + 0x00800080u) >> 8) & kSsrPyrMask;      // f == 0: v itself
            v.g = (v.g * (256u - f) + u.g * f + 128u) >> 8;
        }
        return (v.rb & 255u) | (v.g << 8) | (v.rb & 0x00FF0000u);
    }
};

}  // namespace cry
