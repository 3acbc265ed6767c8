// decal_core.hpp -- the body of crychic_apply_decals (include/crychic_hip.h states the definition), built for
// the device (decal.hip) and for the host (tests/decal_host).  One lane per pixel, an 8 x 8 pixel tile per wavefront:
//   * every lane loads its depth word and, if covered, its G0 texel; the wavefront reduces the box of its covered positions
//     (light_core.hpp's tile_box_pixel / tile_box_merge: a non-finite covered position makes the box all of space);
//   * lane k tests decal k's bounds against that box (decal_tile_test); the vote is the tile's 64-bit decal mask.  Step 2 of the
//     definition is the same compare per pixel, so a decal outside the mask changes no pixel of the tile: the cull is exact;
//   * a mask of 0 ends the wavefront; the others load G1 and G2 and walk the mask's bits in ascending order (decal_lane), the decal
//     index wave-uniform, and store what the definition says is stored.
// A plane's texel is kept as raw words beside its widened value: a component that is not stored is written back with the bits it
// had (a NaN payload, a half that float_to_half(half_to_float(h)) would quieten), and a texel none of whose components is stored
// is not written at all.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "devmath.hpp"
#include "light_core.hpp"

namespace cry {

// a wavefront covers an 8 x 8 pixel tile (lane = 8 y + x), a workgroup four tiles side by side: 32 x 8 pixels (the fog pass's shape)
constexpr uint32_t kDecalTile = 8u, kDecalWaves = 4u, kDecalGroupW = kDecalTile * kDecalWaves, kDecalThreads = 64u * kDecalWaves;
CRY_HD uint32_t decal_lane_x(uint32_t thread) { return (thread >> 6) * kDecalTile + (thread & (kDecalTile - 1u)); }   // within the workgroup
CRY_HD uint32_t decal_lane_y(uint32_t thread) { return (thread >> 3) & (kDecalTile - 1u); }

struct DecalTexture { const uint8_t* rgba8; uint32_t width, height, levels; };        // levels = max(mipLevels, 1)

// the kernel's arguments (kernarg segment: every field is wave-uniform)
struct DecalArgs {
    const uint32_t* depth;
    void* g0;
    void* g1;
    void* g2;
    const crychic_decal* decals;
    uint32_t n, nTextures, W, row0, rowEnd, tilesX, h0, h1, h2;
    float vz[4];            // View + 8
    float pix;              // 2 / (Proj[5] H)
    DecalTexture tex[CRYCHIC_DECAL_MAX_TEXTURES];
};

struct DecalLaunch { DecalArgs args; uint32_t groups; };      // groups == 0: nothing to launch

// The launcher's plan and the host-side constants of the definition.  The caller has checked every argument (api.cpp).
inline DecalLaunch decal_launch(const float* view, const float* proj, const uint32_t* depth, void* g0, void* g1, void* g2, uint32_t formatFlags,
                                const crychic_decal* decals, uint32_t nDecals, const crychic_texture* textures, uint32_t nTextures, uint32_t W,
                                uint32_t H, uint32_t row0, uint32_t rows)
{
    DecalLaunch L;
    DecalArgs& a = L.args;
    a.depth = depth; a.g0 = g0; a.g1 = g1; a.g2 = g2; a.decals = decals;
    a.n = nDecals; a.nTextures = nTextures; a.W = W; a.row0 = row0; a.rowEnd = row0 + rows;
    a.tilesX = (W + kDecalGroupW - 1u) / kDecalGroupW;
    a.h0 = formatFlags & CRYCHIC_GBUFFER_G0_F16; a.h1 = formatFlags & CRYCHIC_GBUFFER_G1_F16; a.h2 = formatFlags & CRYCHIC_GBUFFER_G2_F16;
    for (int k = 0; k < 4; ++k) a.vz[k] = view[8 + k];
    a.pix = 2.0f / (proj[5] * (float)H);
    for (uint32_t k = 0; k < CRYCHIC_DECAL_MAX_TEXTURES; ++k) {
        a.tex[k] = DecalTexture{ nullptr, 1u, 1u, 1u };
        if (k < nTextures) a.tex[k] = DecalTexture{ textures[k].rgba8_dev, textures[k].width, textures[k].height, textures[k].mipLevels > 1u ? textures[k].mipLevels : 1u };
    }
    L.groups = nDecals ? a.tilesX * ((rows + kDecalTile - 1u) / kDecalTile) : 0u;      // below 2^27: fits
    return L;
}

// One texel of a G-buffer plane: its words as they lie in memory (two of them for a half4 plane) and the four values, widened
struct DecalTexel { u4 raw; f4a v; };
CRY_HD DecalTexel decal_load(const void* plane, uint32_t idx, uint32_t isHalf)
{
    DecalTexel t;
    if (isHalf) {
        const u2 r = static_cast<const u2*>(plane)[idx];
        t.raw = u4{ r.x, r.y, 0u, 0u };
        t.v = gbuffer_widen(r);
    } else {
        t.raw = static_cast<const u4*>(plane)[idx];
        t.v = f4a{ u2f(t.raw.x), u2f(t.raw.y), u2f(t.raw.z), u2f(t.raw.w) };
    }
    return t;
}
// Components whose bit of `which` is set (bit c = component c) take `v` in the plane's format, the others keep their bits; which == 0
// stores nothing.
CRY_HD void decal_store(void* plane, uint32_t idx, uint32_t isHalf, u4 raw, f4a v, uint32_t which)
{
    if (!which) return;
    if (isHalf) {
        const uint32_t hx = (which & 1u) ? float_to_half(v.x) : (raw.x & 0xFFFFu), hy = (which & 2u) ? float_to_half(v.y) : (raw.x >> 16);
        const uint32_t hz = (which & 4u) ? float_to_half(v.z) : (raw.y & 0xFFFFu), hw = (which & 8u) ? float_to_half(v.w) : (raw.y >> 16);
        static_cast<u2*>(plane)[idx] = u2{ hx | (hy << 16), hz | (hw << 16) };
    } else {
        static_cast<u4*>(plane)[idx] = u4{ (which & 1u) ? f2u(v.x) : raw.x, (which & 2u) ? f2u(v.y) : raw.y, (which & 4u) ? f2u(v.z) : raw.z,
                                           (which & 8u) ? f2u(v.w) : raw.w };
    }
}

// Lane k's test of decal k: do the decal's bounds meet the tile's box?  Closed on both sides, as step 2 is: for a covered pixel
// that passes step 2, lo <= P <= boundsMax and hi >= P >= boundsMin in every component.  A NaN bound fails here as it fails there;
// a tile without a covered pixel admits nothing.
CRY_HD bool decal_tile_test(const crychic_decal& d, const TileBox& b)
{
    bool hit = tile_box_any_covered(b);
#pragma unroll
    for (int c = 0; c < 3; ++c) hit = hit && b.lo[c] <= d.boundsMax[c] && b.hi[c] >= d.boundsMin[c];
    return hit;
}

// fetch(k): one bilinear CLAMP fetch inside level k.  u and v lie in [0, 1] (step 3 bounds q), so bilinear_setup's non-finite case
// cannot occur and i0 lies in [-1, w - 1].  A level holds at most 2^28 texels (api.cpp), so texel indices fit 32 bits.
CRY_HD f4 decal_fetch(const DecalTexture& t, uint32_t level, float u, float v)
{
    uint32_t w = t.width, h = t.height;
    size_t off = 0;
    for (uint32_t k = 0; k < level; ++k) { off += (size_t)w * h; w = w > 1u ? w >> 1 : 1u; h = h > 1u ? h >> 1 : 1u; }
    const Bilin b = bilinear_setup<true>(u, v, w, h);
    const uint32_t x0 = (uint32_t)clampi(b.i0, 0, (int)w - 1), x1 = (uint32_t)clampi(b.i0 + 1, 0, (int)w - 1);
    const uint32_t y0 = (uint32_t)clampi(b.j0, 0, (int)h - 1), y1 = (uint32_t)clampi(b.j0 + 1, 0, (int)h - 1);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(t.rgba8) + off;
    const uint32_t t00 = p[y0 * w + x0], t10 = p[y0 * w + x1], t01 = p[y1 * w + x0], t11 = p[y1 * w + x1];
    f4 o;
    o.x = bilerp(unorm8_to_float(t00 & 255u), unorm8_to_float(t10 & 255u), unorm8_to_float(t01 & 255u), unorm8_to_float(t11 & 255u), b.fx, b.fy);
    o.y = bilerp(unorm8_to_float((t00 >> 8) & 255u), unorm8_to_float((t10 >> 8) & 255u), unorm8_to_float((t01 >> 8) & 255u), unorm8_to_float((t11 >> 8) & 255u), b.fx, b.fy);
    o.z = bilerp(unorm8_to_float((t00 >> 16) & 255u), unorm8_to_float((t10 >> 16) & 255u), unorm8_to_float((t01 >> 16) & 255u), unorm8_to_float((t11 >> 16) & 255u), b.fx, b.fy);
    o.w = bilerp(unorm8_to_float(t00 >> 24), unorm8_to_float(t10 >> 24), unorm8_to_float(t01 >> 24), unorm8_to_float(t11 >> 24), b.fx, b.fy);
    return o;
}

// sample(T): step 6.  st = s * texelsPerUnit.
CRY_HD f4 decal_sample(const DecalTexture& t, float u, float v, float st)
{
    if (t.levels == 1u) return decal_fetch(t, 0u, u, v);
    const float lod = clampf(det_log2(st), 0.0f, (float)(t.levels - 1u));         // NaN and -inf: 0
    const float l0f = __builtin_floorf(lod), fl = lod - l0f;
    const uint32_t l0 = (uint32_t)l0f, l1 = l0 + 1u < t.levels ? l0 + 1u : t.levels - 1u;
    const f4 a = decal_fetch(t, l0, u, v), b = decal_fetch(t, l1, u, v);
    return f4{ lerpf(a.x, b.x, fl), lerpf(a.y, b.y, fl), lerpf(a.z, b.z, fl), lerpf(a.w, b.w, fl) };
}

// One covered pixel: the walk over the tile's decals and the stores.  T0: the pixel's G0 texel, loaded for the box.  `uniform`: the
// device hands a value every lane holds through readfirstlane so that the decal's fields come by scalar loads; the host returns it.
template <class Uniform>
CRY_HD void decal_lane(const DecalArgs& a, uint32_t idx, const DecalTexel& T0, uint64_t mask, Uniform uniform)
{
    const DecalTexel T1 = decal_load(a.g1, idx, a.h1), T2 = decal_load(a.g2, idx, a.h2);
    const f3 P{ T0.v.x, T0.v.y, T0.v.z };
    const f3 n0 = normalize3(f3{ T2.v.x, T2.v.y, T2.v.z });
    f3 alb{ T1.v.x, T1.v.y, T1.v.z }, nrm = n0;
    float rough = T1.v.w, metal = T0.v.w;
    const float s = mulcol1(P.x, P.y, P.z, a.vz) * a.pix;
    uint32_t stored = 0u;
    while (mask) {
        const uint32_t di = uniform((uint32_t)__builtin_ctzll(mask));
        mask &= mask - 1u;
        const crychic_decal& D = a.decals[di];
        if (D.texture >= a.nTextures) continue;                                                                    // step 1
        if (!(P.x >= D.boundsMin[0] && P.x <= D.boundsMax[0] && P.y >= D.boundsMin[1] && P.y <= D.boundsMax[1] &&
              P.z >= D.boundsMin[2] && P.z <= D.boundsMax[2])) continue;                                           // step 2
        const float qx = mulcol1(P.x, P.y, P.z, D.invWorld), qy = mulcol1(P.x, P.y, P.z, D.invWorld + 4), qz = mulcol1(P.x, P.y, P.z, D.invWorld + 8);
        if (!(__builtin_fabsf(qx) <= 0.5f && __builtin_fabsf(qy) <= 0.5f && __builtin_fabsf(qz) <= 0.5f)) continue;   // step 3
        const float fade = saturate(fma(dot3(n0, f3{ D.normalW[0], D.normalW[1], D.normalW[2] }), D.fadeScale, D.fadeBias));   // step 4
        const float u = qx + 0.5f, v = 0.5f - qy;                                                                  // step 5
        const float st = s * D.texelsPerUnit;
        const f4 t = decal_sample(a.tex[D.texture], u, v, st);                                                     // step 6
        const float al = (t.w * D.opacity) * fade;                                                                 // step 7
        if (!(al > 0.0f)) continue;
        const uint32_t flags = D.flags;
        if (flags & CRYCHIC_DECAL_ALBEDO) {                                                                        // step 8
            alb.x = lerpf(alb.x, t.x * D.tint[0], al);
            alb.y = lerpf(alb.y, t.y * D.tint[1], al);
            alb.z = lerpf(alb.z, t.z * D.tint[2], al);
        }
        if (flags & CRYCHIC_DECAL_ROUGHNESS) rough = lerpf(rough, D.roughness, al);
        if (flags & CRYCHIC_DECAL_METALNESS) metal = lerpf(metal, D.metalness, al);
        const bool mapped = (flags & CRYCHIC_DECAL_NORMAL) && D.normalTexture < a.nTextures;
        if (mapped) {                                                                                              // step 9
            const f4 m = decal_sample(a.tex[D.normalTexture], u, v, st);
            const float ex = fma(m.x, 2.0f, -1.0f), ey = fma(m.y, 2.0f, -1.0f), ez = fma(m.z, 2.0f, -1.0f);
            nrm.x = lerpf(nrm.x, fma(ez, D.normalW[0], fma(ey, D.bitangentW[0], ex * D.tangentW[0])), al);
            nrm.y = lerpf(nrm.y, fma(ez, D.normalW[1], fma(ey, D.bitangentW[1], ex * D.tangentW[1])), al);
            nrm.z = lerpf(nrm.z, fma(ez, D.normalW[2], fma(ey, D.bitangentW[2], ex * D.tangentW[2])), al);
        }
        stored |= (flags & (CRYCHIC_DECAL_ALBEDO | CRYCHIC_DECAL_ROUGHNESS | CRYCHIC_DECAL_METALNESS)) | (mapped ? CRYCHIC_DECAL_NORMAL : 0u);
    }
    decal_store(a.g0, idx, a.h0, T0.raw, f4a{ 0.0f, 0.0f, 0.0f, metal }, (stored & CRYCHIC_DECAL_METALNESS) ? 8u : 0u);
    decal_store(a.g1, idx, a.h1, T1.raw, f4a{ alb.x, alb.y, alb.z, rough },
                ((stored & CRYCHIC_DECAL_ALBEDO) ? 7u : 0u) | ((stored & CRYCHIC_DECAL_ROUGHNESS) ? 8u : 0u));
    decal_store(a.g2, idx, a.h2, T2.raw, f4a{ nrm.x, nrm.y, nrm.z, 0.0f }, (stored & CRYCHIC_DECAL_NORMAL) ? 7u : 0u);
}

}  // namespace cry
