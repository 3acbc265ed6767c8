// point_shadow_host.cpp -- TEST HARNESS ONLY.  The shadowed point-light kernel body (csrc/light_core.hpp light_pixel with the
// AllLocalLights functor and its pointShadows: pbr_point_light with PointShadowOf, then pbr_spot_light) compiled for the host CPU, so
// that the CPU-only tier checks it bit for bit against tests/point_shadow_ref/point_shadow_ref.c.  pointShadowCount 0 models the
// kernels without point shadows (tests/local_light_ref/local_light_host.cpp), otherwise light_point_shadows_kernel.  The tiled
// kernel walks the culled lights in the same ascending order as the un-culled iteration here.
#include <cstring>
#include "light_core.hpp"

using namespace cry;

extern "C" int psh_point_face(const float v[3], float abc[3])
{
    const PointFace pf = point_face(f3{ v[0], v[1], v[2] });
    abc[0] = pf.abc.x; abc[1] = pf.abc.y; abc[2] = pf.abc.z;
    return (int)pf.f;
}

// shadowProj: 16 floats, untransposed (crychic_update_point_shadow_transforms)
extern "C" float psh_point_shadow_factor(const uint32_t* faces, uint32_t dim, const float shadowProj[16], const float lightPos[3],
                                         const float pos[3])
{
    PointShadows S;
    std::memset(&S, 0, sizeof S);
    S.maps[0] = faces;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) S.M[0][4 * i + j] = shadowProj[4 * j + i];
    S.count = 1; S.dim = dim; S.dx = 1.0f / (float)dim;
    crychic_light L;
    std::memset(&L, 0, sizeof L);
    std::memcpy(L.Position, lightPos, sizeof L.Position);
    return PointShadowOf{ &S, f3{ pos[0], pos[1], pos[2] }, &L, 0u }();
}

extern "C" void psh_light_point_shadows(const crychic_pass_constants* cb, const float* g0, const float* g1, const float* g2,
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
    SpotShadows S;                                          // as api.cpp bind_local_lights builds it
    std::memset(&S, 0, sizeof S);
    for (uint32_t k = 0; k < shadowCount; ++k) { S.maps[k] = shadowMaps[k]; std::memcpy(S.T[k], cb->ShadowTransforms[4 + k], sizeof S.T[k]); }
    S.count = shadowCount; S.dim = shadowMapDim; S.dx = shadowCount ? 1.0f / (float)shadowMapDim : 0.0f;
    PointShadows PS;                                        // as api.cpp bind_local_lights builds it (shadowProj transposed)
    std::memset(&PS, 0, sizeof PS);
    for (uint32_t k = 0; k < pointShadowCount; ++k) {
        PS.maps[k] = pointMaps[k];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) PS.M[k][4 * i + j] = shadowProj[16 * k + 4 * j + i];
    }
    PS.count = pointShadowCount; PS.dim = pointShadowDim; PS.dx = pointShadowCount ? 1.0f / (float)pointShadowDim : 0.0f;
    // light_point_shadows_kernel takes the spot lights with their shadow functor even at a spot shadow count of 0 (factor 1)
    const AllLocalLights ll{ pointLights, numPointLights, spotLights, numSpotLights, (shadowCount || pointShadowCount) ? &S : nullptr,
                             pointShadowCount ? &PS : nullptr };
    const f4a* G0 = (const f4a*)g0; const f4a* G1 = (const f4a*)g1; const f4a* G2 = (const f4a*)g2;
    auto shaded = [&](uint32_t xx, uint32_t yy) { return xx < W && yy < row0 + rows && (depth[yy * W + xx] & 0x00FFFFFFu) < 0x00FFFFFFu; };
    for (uint32_t y = row0; y < row0 + rows; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t idx = y * W + x;
            f4 lit;
            if (shaded(x, y) && chain) {
                // light_point_shadows_kernel<.., MIPS>: the quad neighbours' reflection vectors by lane exchange there, by recomputation here
                const f3 r = reflection_dir(P, G0[idx], G2[idx]);
                f3 ddx{ 0.0f, 0.0f, 0.0f }, ddy{ 0.0f, 0.0f, 0.0f };
                if (shaded(x ^ 1u, y)) { const f3 n = reflection_dir(P, G0[y * W + (x ^ 1u)], G2[y * W + (x ^ 1u)]); ddx = (x & 1u) ? f3{ r.x - n.x, r.y - n.y, r.z - n.z } : f3{ n.x - r.x, n.y - r.y, n.z - r.z }; }
                if (shaded(x, y ^ 1u)) { const f3 n = reflection_dir(P, G0[(y ^ 1u) * W + x], G2[(y ^ 1u) * W + x]); ddy = (y & 1u) ? f3{ r.x - n.x, r.y - n.y, r.z - n.z } : f3{ n.x - r.x, n.y - r.y, n.z - r.z }; }
                const float lod = cube_lod(P.cubeDim, P.cubeLevels, r, ddx, ddy);
                const CubeChain cc{ lod, cube_chain_flat(lod) };
                if (pcfSearchRadius == 0.0f) lit = light_pixel<true, AllLocalLights, true, CubeChain>(P, G0[idx], G1[idx], G2[idx], ambient, (const uint32_t*)cube, ll, cc);
                else lit = light_pixel<false, AllLocalLights, true, CubeChain>(P, G0[idx], G1[idx], G2[idx], ambient, (const uint32_t*)cube, ll, cc);
            } else if (shaded(x, y)) {
                // the spot kernels compile FIX in, as the point-light kernel does
                if (pcfSearchRadius == 0.0f) lit = light_pixel<true, AllLocalLights, true>(P, G0[idx], G1[idx], G2[idx], ambient, (const uint32_t*)cube, ll);
                else lit = light_pixel<false, AllLocalLights, true>(P, G0[idx], G1[idx], G2[idx], ambient, (const uint32_t*)cube, ll);
            }
            else if (flags & CRYCHIC_LIGHT_SKY) lit = chain ? sky_pixel_chain(P, (const uint32_t*)cube, x, y) : sky_pixel(P, (const uint32_t*)cube, x, y);
            else lit = f4{ 0.690196097f, 0.768627524f, 0.870588303f, 1.0f };
            if (radiance) { radiance[4 * idx] = lit.x; radiance[4 * idx + 1] = lit.y; radiance[4 * idx + 2] = lit.z; radiance[4 * idx + 3] = lit.w; }
            ((uint32_t*)out)[idx] = pack_rgba8(lit);
        }
}
