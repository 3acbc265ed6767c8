// gbuffer_f16_host.cpp -- TEST HARNESS ONLY.  The G-buffer plane formats (include/crychic_hip.h CRYCHIC_GBUFFER_G*_F16) compiled for
// the host CPU, so that the CPU-only tier checks them bit for bit before any GPU time is spent:
//   gfh_light      the format-aware load (csrc/light_core.hpp gbuffer_load: a half4 texel through half_to_float) in front of
//                  light_pixel, as light_formats_kernel (no local lights) and light_point_shadows_formats_kernel (any) run it;
//   gfh_rasterize  the producer passes with the format-aware resolve (csrc/raster_core.hpp gbuffer_store: four float_to_half packed
//                  into one 8-byte texel), as resolve_formats_kernel runs it.
// Modelled on tests/point_shadow_ref/point_shadow_host.cpp and tests/hostsim/hostsim.cpp (hs_rasterize).
#include <cstring>
#include <vector>
#include "light_core.hpp"
#include "raster_core.hpp"

using namespace cry;

extern "C" uint16_t gfh_float_to_half(float f) { return float_to_half(f); }
extern "C" float gfh_half_to_float(uint16_t h) { return half_to_float(h); }

// g0 / g1 / g2: float4 or half4 texels by the CRYCHIC_GBUFFER_G*_F16 bits of flags.
extern "C" void gfh_light(const crychic_pass_constants* cb, const void* g0, const void* g1, const void* g2,
                          const uint32_t* depth, const uint16_t* ambient, const uint32_t* const shadow[4], uint32_t shadowDim,
                          const uint8_t* cube, uint32_t cubeDim, uint8_t* out, float* radiance, uint32_t W, uint32_t H,
                          uint32_t row0, uint32_t rows, int numDirLights, float pcfSearchRadius, uint32_t flags,
                          const crychic_light* pointLights, uint32_t numPointLights, const crychic_light* spotLights,
                          uint32_t numSpotLights, uint32_t shadowCount, uint32_t shadowMapDim, const uint32_t* const* shadowMaps,
                          uint32_t pointShadowCount, uint32_t pointShadowDim, const uint32_t* const* pointMaps, const float* shadowProj)
{
    LightParams P;
    std::memcpy(P.ViewProjTex, cb->ViewProjTex, sizeof P.ViewProjTex);
    std::memcpy(P.ShadowTransforms, cb->ShadowTransforms, sizeof P.ShadowTransforms);
    std::memcpy(P.InvProj, cb->InvProj, sizeof P.InvProj);
    std::memcpy(P.InvView, cb->InvView, sizeof P.InvView);
    std::memcpy(P.EyePosW, cb->EyePosW, sizeof P.EyePosW);
    P.pcfSearchRadius = pcfSearchRadius;
    std::memcpy(P.AmbientLight, cb->AmbientLight, sizeof P.AmbientLight);
    std::memcpy(P.Lights, cb->Lights, sizeof P.Lights);
    for (int i = 0; i < 4; ++i) P.shadow[i] = shadow[i];
    P.shadowDim = shadowDim; P.cubeDim = cubeDim; P.W = W; P.H = H; P.numDirLights = numDirLights; P.flags = flags;
    P.pointLights = pointLights; P.numPointLights = numPointLights;
    P.shadowWIsOne = light_shadow_w_is_one(P.ShadowTransforms) ? 1u : 0u;
    P.darkLights = light_dark_mask(P.Lights, numDirLights);
    P.unitLights = light_dark_lengths_ok(P.Lights, numDirLights) ? 1u : 0u;
    P.rcpW = rcp((float)W); P.rcpH = rcp((float)H);
    P.cubeLevels = (flags >> 16) & 15u;                    // CRYCHIC_LIGHT_CUBE_LEVELS
    light_params_derive(P);
    const bool chain = P.cubeLevels > 1u;
    SpotShadows S;                                          // as api.cpp bind_local_lights builds them
    std::memset(&S, 0, sizeof S);
    for (uint32_t k = 0; k < shadowCount; ++k) { S.maps[k] = shadowMaps[k]; std::memcpy(S.T[k], cb->ShadowTransforms[4 + k], sizeof S.T[k]); }
    S.count = shadowCount; S.dim = shadowMapDim; S.dx = shadowCount ? 1.0f / (float)shadowMapDim : 0.0f;
    PointShadows PS;
    std::memset(&PS, 0, sizeof PS);
    for (uint32_t k = 0; k < pointShadowCount; ++k) {
        PS.maps[k] = pointMaps[k];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) PS.M[k][4 * i + j] = shadowProj[16 * k + 4 * j + i];
    }
    PS.count = pointShadowCount; PS.dim = pointShadowDim; PS.dx = pointShadowCount ? 1.0f / (float)pointShadowDim : 0.0f;
    // launch_light_formats: any local light takes light_point_shadows_formats_kernel, which carries both shadow functors whatever the counts
    const bool local = numPointLights || numSpotLights;
    const AllLocalLights ll{ pointLights, numPointLights, spotLights, numSpotLights, &S, &PS };
    const uint32_t h0 = flags & CRYCHIC_GBUFFER_G0_F16, h1 = flags & CRYCHIC_GBUFFER_G1_F16, h2 = flags & CRYCHIC_GBUFFER_G2_F16;
    auto shaded = [&](uint32_t xx, uint32_t yy) { return xx < W && yy < row0 + rows && (depth[yy * W + xx] & 0x00FFFFFFu) < 0x00FFFFFFu; };
    auto reflection = [&](uint32_t xx, uint32_t yy) { return reflection_dir(P, gbuffer_load(g0, yy * W + xx, h0), gbuffer_load(g2, yy * W + xx, h2)); };
    const uint32_t* cubeTexels = (const uint32_t*)cube;
    for (uint32_t y = row0; y < row0 + rows; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t idx = y * W + x;
            f4 lit;
            if (shaded(x, y)) {
                const f4a G0 = gbuffer_load(g0, idx, h0), G1 = gbuffer_load(g1, idx, h1), G2 = gbuffer_load(g2, idx, h2);
                CubeChain cc{ 0.0f, true };
                if (chain) {        // <.., MIPS>: the quad neighbours' reflection vectors by lane exchange there, by recomputation here
                    const f3 r = reflection_dir(P, G0, G2);
                    f3 ddx{ 0.0f, 0.0f, 0.0f }, ddy{ 0.0f, 0.0f, 0.0f };
                    if (shaded(x ^ 1u, y)) { const f3 n = reflection(x ^ 1u, y); ddx = (x & 1u) ? f3{ r.x - n.x, r.y - n.y, r.z - n.z } : f3{ n.x - r.x, n.y - r.y, n.z - r.z }; }
                    if (shaded(x, y ^ 1u)) { const f3 n = reflection(x, y ^ 1u); ddy = (y & 1u) ? f3{ r.x - n.x, r.y - n.y, r.z - n.z } : f3{ n.x - r.x, n.y - r.y, n.z - r.z }; }
                    const float lod = cube_lod(P.cubeDim, P.cubeLevels, r, ddx, ddy);
                    cc = CubeChain{ lod, cube_chain_flat(lod) };
                }
                const bool zero = pcfSearchRadius == 0.0f;
                if (local && chain) lit = zero ? light_pixel<true, AllLocalLights, true, CubeChain>(P, G0, G1, G2, ambient, cubeTexels, ll, cc)
                                               : light_pixel<false, AllLocalLights, true, CubeChain>(P, G0, G1, G2, ambient, cubeTexels, ll, cc);
                else if (local) lit = zero ? light_pixel<true, AllLocalLights, true>(P, G0, G1, G2, ambient, cubeTexels, ll)
                                           : light_pixel<false, AllLocalLights, true>(P, G0, G1, G2, ambient, cubeTexels, ll);
                else if (chain) lit = zero ? light_pixel<true, NoPointLights, true, CubeChain>(P, G0, G1, G2, ambient, cubeTexels, NoPointLights(), cc)
                                           : light_pixel<false, NoPointLights, true, CubeChain>(P, G0, G1, G2, ambient, cubeTexels, NoPointLights(), cc);
                else lit = zero ? light_pixel<true, NoPointLights, true>(P, G0, G1, G2, ambient, cubeTexels)
                                : light_pixel<false, NoPointLights, true>(P, G0, G1, G2, ambient, cubeTexels);
            }
            else if (flags & CRYCHIC_LIGHT_SKY) lit = chain ? sky_pixel_chain(P, cubeTexels, x, y) : sky_pixel(P, cubeTexels, x, y);
            else lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
            if (radiance) { radiance[4 * idx] = lit.x; radiance[4 * idx + 1] = lit.y; radiance[4 * idx + 2] = lit.z; radiance[4 * idx + 3] = lit.w; }
            ((uint32_t*)out)[idx] = pack_rgba8(lit);
        }
}

// crychic_draw_gbuffer_formats on the host: hs_rasterize's sequence (setup in draw order into setup_kernel's slot numbering, coverage
// by min() on the 64-bit key) with resolve_formats_kernel's stage.  normal == NULL: the G-buffer pass alone (mode 2: depth and G0..G2
// for rows [gRow0, gRow0 + gRows) only), otherwise the fused pass (mode 3: depth and normals everywhere, G0..G2 in the rows).
// gRows == 0: the whole target.  Texels the pass does not write are left as they are.
extern "C" int gfh_rasterize(const float* view, const float* viewProj, const crychic_draw_item* items, uint32_t nItems,
                             const crychic_material_data* materials, uint32_t nMaterials, const crychic_texture* textures, uint32_t nTextures,
                             uint32_t W, uint32_t H, uint32_t* depth, uint16_t* normal, void* g0, void* g1, void* g2, uint32_t gbufferFlags,
                             uint32_t gRow0, uint32_t gRows)
{
    const int passMode = normal ? 3 : 2;
    const uint32_t gLo = gRows ? gRow0 : 0u, gHi = gRows ? gRow0 + gRows : H;
    const uint32_t yLo = passMode == 2 ? gLo : 0u, yHi = passMode == 2 ? gHi : H;
    std::vector<SetupTri> tris;
    bool overflow = false;
    for (uint32_t it = 0; it < nItems; ++it) {
        const crychic_draw_item& d = items[it];
        const uint32_t ntri = d.indexCount / 3u;
        for (uint32_t inst = 0; inst < d.instanceCount; ++inst)
            for (uint32_t tri = 0; tri < ntri; ++tri) {
                const crychic_instance_data& I = d.instances_dev[inst];
                const crychic_material_data* M = (materials && I.MaterialIndex < nMaterials) ? &materials[I.MaterialIndex] : nullptr;
                const size_t slot0 = tris.size();
                tris.resize(slot0 + kSlotsPerTriangle);
                for (int c = 0; c < kSlotsPerTriangle; ++c) tris[slot0 + (size_t)c].A2 = 0;
                VsOut poly[kMaxPolyVerts], tmp[kMaxPolyVerts];
                for (int c = 0; c < 3; ++c) {
                    const int64_t vi = (int64_t)d.indices_dev[d.startIndexLocation + tri * 3u + c] + d.baseVertexLocation;
                    if (vi < 0 || vi >= (int64_t)d.vertexCount) return -1;
                    poly[c] = vertex_shader(d.vertices_dev[vi], I, M, viewProj);
                }
                const int n = clip_triangle(poly, tmp, W, H);
                for (int c = 1; c + 1 < n; ++c) {
                    SetupTri s;
                    if (setup_triangle(poly[0], poly[c], poly[c + 1], I.MaterialIndex, W, H, s, &overflow)) tris[slot0 + (size_t)(c - 1)] = s;
                }
            }
    }
    if (overflow) return -2;
    std::vector<uint64_t> vis((size_t)W * H, kVisClear);
    int live = 0;
    for (size_t slot = 0; slot < tris.size(); ++slot) {
        const SetupTri& t = tris[slot];
        if (t.A2 <= 0) continue;
        ++live;
        const PixelBox b = triangle_box(t, W, yLo, yHi);
        const EdgeFlags e = triangle_edge_flags(t);
        for (int y = b.y0; y <= b.y1; ++y)
            for (int x = b.x0; x <= b.x1; ++x) {
                const uint64_t key = fragment_key(t, e, 0.0, x, y, (uint32_t)slot + 1u);
                uint64_t& v = vis[(size_t)y * W + x];
                if (key < v) v = key;
            }
    }
    const Texture* tex = reinterpret_cast<const Texture*>(textures);
    const uint32_t h0 = gbufferFlags & CRYCHIC_GBUFFER_G0_F16, h1 = gbufferFlags & CRYCHIC_GBUFFER_G1_F16, h2 = gbufferFlags & CRYCHIC_GBUFFER_G2_F16;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            int mode = passMode;
            if (y < gLo || y >= gHi) { mode &= ~2; if (mode == 0) continue; }
            const uint32_t idx = y * W + x;
            const uint64_t key = vis[idx];
            const uint32_t serial = (uint32_t)(key & 0xFFFFFFFFull);
            depth[idx] = (uint32_t)(key >> 32);
            if (serial == 0) {
                if (mode & 1) { normal[idx * 4] = 0; normal[idx * 4 + 1] = 0; normal[idx * 4 + 2] = 0x3C00; normal[idx * 4 + 3] = 0; }
                if (mode & 2) { const f4 zero{ 0.0f, 0.0f, 0.0f, 0.0f }; gbuffer_store(g0, idx, h0, zero); gbuffer_store(g1, idx, h1, zero); gbuffer_store(g2, idx, h2, zero); }
                continue;
            }
            const ResolveOut r = resolve_pixel(mode, tris[serial - 1u], (int)x, (int)y, view, materials, nMaterials, tex, nTextures);
            if (mode & 1) {
                normal[idx * 4] = float_to_half(r.normalV.x); normal[idx * 4 + 1] = float_to_half(r.normalV.y);
                normal[idx * 4 + 2] = float_to_half(r.normalV.z); normal[idx * 4 + 3] = 0;
            }
            if (mode & 2) { gbuffer_store(g0, idx, h0, r.g0); gbuffer_store(g1, idx, h1, r.g1); gbuffer_store(g2, idx, h2, r.g2); }
        }
    return live;
}
