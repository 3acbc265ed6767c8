// kernels.hpp -- launcher interface between the C ABI (api.cpp) and the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "crychic_hip.h"

namespace cry {

struct LightParams;
struct SpotShadows;
struct PointShadows;

// Launch grid of the full-screen passes: a workgroup per 64 pixels x rows_per_block rows (shared by kernels.hip and light_general.hip).
inline dim3 grid_for(uint32_t width, uint32_t rows, uint32_t rows_per_block = 4u)
{
    return dim3((width + 63u) / 64u, (rows + rows_per_block - 1u) / rows_per_block, 1);
}

// D24 depth plane -> the decoded, BORDER-padded pairs plane inside the edge workspace (ssao_core.hpp "depth pairs") and the coarse
// maps of the SSAO shortcuts, for the SSAO pass over half-res rows [row0, row0 + rows): those rows' texels and a margin (the whole
// plane when the rows are the whole map; launch_ssao called with the same rows knows what was prepared).
// `stamp` (non-zero, different from the previous frame's) marks the cells of the coarse geometry map written by this call.
hipError_t launch_depth_pairs(const crychic_ssao_constants& cb, const uint32_t* depth, void* edge_base, uint32_t W, uint32_t H, uint32_t stamp,
                              bool writePairs, uint32_t row0, uint32_t rows, hipStream_t stream);
// use_pairs: the taps read the pairs plane (launch_depth_pairs earlier on the same stream) instead of the raw D24 plane.
hipError_t launch_ssao(const crychic_ssao_constants& cb, const void* normal, const uint32_t* depth,
                       const uint8_t* randvec, uint16_t* ambient, void* edge_base, uint32_t W, uint32_t H,
                       uint32_t row0, uint32_t rows, bool emit_ao, bool use_pairs, uint32_t stamp, hipStream_t stream);

// One self-contained sweep of SsaoBlur.hlsl (Ssao::BlurAmbientMap(cmdList, bool), Ssao.cpp:245-293) over half-res rows [row0, row0 + rows).
hipError_t launch_blur(const crychic_ssao_constants& cb, const void* edge_base, const uint16_t* in, uint16_t* out,
                       uint32_t W, uint32_t H, bool horizontal, uint32_t row0, uint32_t rows, hipStream_t stream);
// Iteration 0 of the blur chain: horizontal + vertical sweep in one launch (in -> out, out != in); the rows are those of the
// vertical sweep's output.  record: store both sweeps' tap decisions and the per-tile flags for launch_blur_replay.
// stamp (0 = no exit) / onesMargin / ssaoRow0, ssaoRows: the unoccluded-tile exit (blur_tiles.hpp) -- the SSAO pass of this frame
// wrote the unoccluded-wavefront map with `stamp` for half-res rows [ssaoRow0, ssaoRow0 + ssaoRows).
hipError_t launch_blur_pair(const crychic_ssao_constants& cb, const void* edge_base, const uint16_t* in, uint16_t* out, uint32_t W, uint32_t H,
                            uint32_t row0, uint32_t rows, bool record, uint32_t stamp, int onesMargin, uint32_t ssaoRow0, uint32_t ssaoRows,
                            hipStream_t stream);
// A later iteration of the chain (both sweeps), replaying what launch_blur_pair(record) stored (in -> out, out != in); the rows
// are those owed after it.  stamp: the one the pair launch ran with (its settled tiles return at once).
hipError_t launch_blur_replay(const crychic_ssao_constants& cb, const void* edge_base, const uint16_t* in, uint16_t* out, uint32_t W, uint32_t H,
                              uint32_t row0, uint32_t rows, uint32_t stamp, hipStream_t stream);

// Iterations 1 .. blurCount - 1 of the chain in one launch (kernels.hip blur_replay_chain_kernel: per-tile dependencies instead of
// kernel boundaries); plane0 / plane1 = ambient0 / ambient1, rows = what the caller is owed of the final map, stamp = the frame's
// (the one launch_blur_pair ran with).  Same pixels as blurCount - 1 calls of launch_blur_replay along blur_chain_step.
hipError_t launch_blur_replay_chain(const crychic_ssao_constants& cb, const void* edge_base, uint16_t* plane0, uint16_t* plane1, uint32_t W, uint32_t H,
                                    int blurCount, uint32_t row0, uint32_t rows, uint32_t stamp, hipStream_t stream);

// spots / numSpots (<= 1024): spot lights after P's point lights (light_spots_kernel); 0 = the point-light or reference kernels.
// shadows: the first shadows->count spot lights shadowed (light_spots_shadowed_kernel); nullptr or count 0 = none.
// pointShadows: the first pointShadows->count point lights shadowed (light_point_shadows_kernel, which takes the spot lights and
// their shadows as well); nullptr or count 0 = the kernels above.
// A CRYCHIC_GBUFFER_G*_F16 bit in P.flags: that plane's pointer addresses half4 texels, and the call goes to launch_light_general.
hipError_t launch_light(const LightParams& P, const float* g0, const float* g1, const float* g2,
                        const uint32_t* depth, const uint16_t* ambient, const uint8_t* cube, uint8_t* out,
                        float* radiance, uint32_t row0, uint32_t rows, hipStream_t stream, const crychic_light* spots,
                        uint32_t numSpots, const SpotShadows* shadows, const PointShadows* pointShadows);
// light_general.hip: the same pass for every call of the general family (light_bind.hpp: a CRYCHIC_GBUFFER_G*_F16 bit,
// CRYCHIC_LIGHT_CUBE_GLOSS, CRYCHIC_LIGHT_AMBIENT_SH or CRYCHIC_LIGHT_ENV_BRDF in P.flags) -- light_general_kernel for a frame without
// local lights, light_general_local_kernel for every other, instantiated by the call's LightVariant; planes of any format mix.  The
// environment terms are read behind the cube map at light_variant_tail's offset.
hipError_t launch_light_general(const LightParams& P, const void* g0, const void* g1, const void* g2, const uint32_t* depth,
                                const uint16_t* ambient, const uint8_t* cube, uint8_t* out, float* radiance, uint32_t row0, uint32_t rows,
                                hipStream_t stream, const crychic_light* spots, uint32_t numSpots, const SpotShadows* shadows,
                                const PointShadows* pointShadows);

// cube_mips.hip: levels 1 .. levels - 1 of an RGBA8 cube map's chain from its level 0, in place (cube_mips_core.hpp); one launch per
// six levels on `stream`.  The caller has checked dim and levels.
hipError_t launch_cube_mips(uint8_t* chain, uint32_t dim, uint32_t levels, hipStream_t stream);

// cube_prefilter.hip: level 0 of `src` copied to `dst` and levels 1 .. levels - 1 of `dst` prefiltered from the chain `src`
// (cube_prefilter_core.hpp); one copy and one launch per level on `stream`.  The caller has checked dim, levels and the overlap.
hipError_t launch_cube_prefilter(const uint8_t* src, uint8_t* dst, uint32_t dim, uint32_t levels, hipStream_t stream);

// cube_sh.hip: the SH9 irradiance coefficients of the six d x d faces at `level` into the environment tail `tail`
// (cube_sh_core.hpp); three launches on `stream`.  The caller has checked d, the alignments and the overlap.
hipError_t launch_cube_sh(const uint8_t* level, uint32_t d, void* tail, hipStream_t stream);
// ... and the probe volume of the box-projected reflection lookup (pos, boxMin, boxMax as three float4) into bytes [368, 416) of
// the environment tail `tail`; one launch on `stream`.  The caller has checked the pointers, the alignment and the values.
hipError_t launch_cube_probe_volume(void* tail, const float pos[3], const float boxMin[3], const float boxMax[3], hipStream_t stream);

// env_brdf.hip: the 32 x 32 environment BRDF table (env_brdf_core.hpp) into the 4096 bytes at `table`; one launch on `stream`.  The
// caller has checked the pointer and its alignment.
hipError_t launch_env_brdf(void* table, hipStream_t stream);

// sky.hip: level 0 of faces [face0, face0 + faces) of the dim-texel cube map `cube` from the atmosphere of `p` (sky_core.hpp); one
// launch on `stream`, none for faces == 0.  The caller has checked the pointer, its alignment, dim, the face range and `p`.
struct SkyParams;
hipError_t launch_sky(uint8_t* cube, uint32_t dim, uint32_t face0, uint32_t faces, const SkyParams& p, hipStream_t stream);

// post_aa.hip: rows [row0, row0 + rows) of the anti-aliased W x H RGBA8 frame `out` from `in` (post_aa_core.hpp); one launch on
// `stream`, none for rows == 0.  The caller has checked the pointers, their alignment and overlap, the sizes, the rows and `p`.
struct PostAaParams;
hipError_t launch_post_aa(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const PostAaParams& p,
                          hipStream_t stream);

// fog.hip: rows [row0, row0 + rows) of the fogged W x H RGBA8 frame `out` from `in`, the D24 plane `depth` and the four dim x dim
// cascade maps (fog_core.hpp); invViewProj, eye and shadowTransforms are the pass constants' fields, read before the call returns.
// One launch on `stream`, none for rows == 0.  The caller has checked the pointers, their alignment and overlap, the sizes, the rows,
// the transforms and `p`.
struct FogParams;
hipError_t launch_fog(const float* invViewProj, const float* eye, const float (*shadowTransforms)[16], const uint32_t* depth,
                      const uint32_t* const* maps, uint32_t dim, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                      uint32_t rows, const FogParams& p, hipStream_t stream);

// ssr.hip: rows [row0, row0 + rows) of the W x H RGBA8 frame `out`: `in` with its own screen-space reflections blended over it, from
// the D24 plane `depth` and the G-buffer planes (half4 where formatFlags has the plane's CRYCHIC_GBUFFER_G*_F16 bit) (ssr_core.hpp);
// proj, viewProj, invViewProj, eye and nearZ are the pass constants' fields, read before the call returns.  One launch on `stream`,
// none for rows == 0.  The caller has checked the pointers, their alignment and overlap, the sizes, the rows, proj and `p`.
struct SsrParams;
hipError_t launch_ssr(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, float nearZ, const void* g0,
                      const void* g1, const void* g2, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H,
                      uint32_t row0, uint32_t rows, uint32_t formatFlags, const SsrParams& p, hipStream_t stream);

// ssr_pyramid.hip: levels 1 .. n_eff of the pyramid of the W x H RGBA8 frame `in` into `workspace` (ssr_pyramid_core.hpp): n_eff
// launches on `stream`, one behind the other, none for n_eff == 0.  ssr_gloss.hip: launch_ssr with the hit colour from that pyramid
// (`pyramid`: the workspace, built with g.levels) by the cone of `g` (ssr_gloss_core.hpp); one launch, none for rows == 0.  The caller
// has checked what launch_ssr's has, and `levels`, `g`, the workspace's alignment, size and overlap.
struct SsrGlossParams;
hipError_t launch_ssr_pyramid(const uint8_t* in, uint32_t W, uint32_t H, uint32_t levels, void* workspace, hipStream_t stream);
hipError_t launch_ssr_glossy(const float* proj, const float* viewProj, const float* invViewProj, const float* eye, float nearZ, const void* g0,
                             const void* g1, const void* g2, const uint32_t* depth, const uint8_t* in, const void* pyramid, uint8_t* out, uint32_t W,
                             uint32_t H, uint32_t row0, uint32_t rows, uint32_t formatFlags, const SsrParams& p, const SsrGlossParams& g,
                             hipStream_t stream);

// dof.hip: rows [row0, row0 + rows) of the W x H RGBA8 frame `out`: `in` blurred by the circle of confusion of the D24 plane `depth`
// (dof_core.hpp); proj is the pass constants' Proj, read before the call returns.  One launch on `stream`, none for rows == 0.  The
// caller has checked the pointers, their alignment and overlap, the sizes, the rows, proj and `p`.
struct DofParams;
hipError_t launch_dof(const float* proj, const uint32_t* depth, const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0,
                      uint32_t rows, const DofParams& p, hipStream_t stream);

// decal.hip: rows [row0, row0 + rows) of the W x H G-buffer planes g0, g1, g2 (half4 where formatFlags has the plane's
// CRYCHIC_GBUFFER_G*_F16 bit) with the nDecals decals of the device array blended in (decal_core.hpp); view and proj are the pass
// constants' fields and textures the host table, all read before the call returns.  One launch on `stream`, none for nDecals == 0 or
// rows == 0.  The caller has checked the pointers, their alignment, the sizes, the rows, the counts, the textures and the constants.
hipError_t launch_decals(const float* view, const float* proj, const uint32_t* depth, void* g0, void* g1, void* g2, uint32_t formatFlags,
                         const crychic_decal* decals, uint32_t nDecals, const crychic_texture* textures, uint32_t nTextures, uint32_t W, uint32_t H,
                         uint32_t row0, uint32_t rows, hipStream_t stream);

// bloom.hip: launch_bloom_pyramid leaves U_k in level k = 1 .. n_eff of `workspace` from the W x H RGBA8 frame `in` (bloom_core.hpp):
// n_eff downsample launches and n_eff - 1 unwind launches on `stream`, one behind the other.  launch_bloom_composite writes rows
// [row0, row0 + rows) of `out` from `in` and level 1 of `workspace`: one launch, none for rows == 0; in == out is in place.  The
// caller has checked the pointers, their alignment and overlap, the sizes, the rows, the workspace's size and `p`.
struct BloomParams;
hipError_t launch_bloom_pyramid(const uint8_t* in, uint32_t W, uint32_t H, const BloomParams& p, void* workspace, hipStream_t stream);
hipError_t launch_bloom_composite(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const BloomParams& p,
                                  const void* workspace, hipStream_t stream);

// taa.hip: rows [row0, row0 + rows) of the W x H RGBA8 frame `out` and of the history plane `historyOut` from `in`, the D24 plane
// `depth` and the history plane `historyIn` (NULL only with the reset flag) (taa_core.hpp); the three matrices are read before the
// call returns.  One launch on `stream`, none for rows == 0.  The caller has checked the pointers, their alignment and overlap, the
// sizes, the rows, the matrices and `p`.
struct TaaParams;
hipError_t launch_taa(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, const uint8_t* in,
                      const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                      const TaaParams& p, hipStream_t stream);

// taa_upscale.hip: rows [row0, row0 + rows) of the Wo x Ho RGBA8 frame `out` and of the history plane `historyOut` from the Wi x Hi
// frame `in`, its D24 plane `depth` and the Wo x Ho history plane `historyIn` (NULL only with the reset flag) (taa_upscale_core.hpp);
// the three matrices are read before the call returns.  One launch on `stream`, none for rows == 0.  The caller has checked the
// pointers, their alignment and overlap, the sizes and their ratios, the rows, the matrices, the jitter and `p`.
struct TaaUpscaleParams;
hipError_t launch_taa_upscale(const float* invViewProj, const float* curViewProj, const float* prevViewProj, float jx, float jy, const uint32_t* depth,
                              const uint8_t* in, uint32_t Wi, uint32_t Hi, const uint16_t* historyIn, uint16_t* historyOut, uint8_t* out, uint32_t Wo,
                              uint32_t Ho, uint32_t row0, uint32_t rows, const TaaUpscaleParams& p, hipStream_t stream);

// motion_blur.hip: launch_motion_blur_velocity fills the velocity plane and the tile plane of `workspace` for the whole W x H frame
// from the D24 plane `depth` (motion_blur_core.hpp); the three matrices are read before the call returns.  launch_motion_blur_gather
// writes rows [row0, row0 + rows) of `out` from `in` and the workspace: none for rows == 0.  One launch each on `stream`.  The caller
// has checked the pointers, their alignment and overlap, the sizes, the rows, the workspace's size and `p`.
struct MotionBlurParams;
hipError_t launch_motion_blur_velocity(const float* invViewProj, const float* curViewProj, const float* prevViewProj, const uint32_t* depth, uint32_t W,
                                       uint32_t H, const MotionBlurParams& p, void* workspace, hipStream_t stream);
hipError_t launch_motion_blur_gather(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const MotionBlurParams& p,
                                     const void* workspace, hipStream_t stream);

// grade.hip: rows [row0, row0 + rows) of the W x H RGBA8 frame `out`: `in` through the N x N x N table `lut` of device memory
// (grade_core.hpp); in == out is in place.  One launch on `stream` with 4 N^3 bytes of LDS, none for rows == 0; a launch the runtime
// refuses comes back as its error code.  The caller has checked the pointers, their alignment and overlap, the sizes, the rows and N.
hipError_t launch_grade(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const uint8_t* lut, uint32_t N,
                        hipStream_t stream);

// sharpen.hip: rows [row0, row0 + rows) of the W x H RGBA8 frame `out` from `in` sharpened (sharpen_core.hpp); neighbours are clamped
// to the frame, not to the rows.  One launch on `stream`, none for rows == 0: the wide kernel where W is a multiple of 4 and both
// planes are 16-byte aligned, the narrow one otherwise.  The caller has checked the pointers, their alignment and overlap, the sizes,
// the rows and the parameters.
struct SharpenParams;
hipError_t launch_sharpen(const uint8_t* in, uint8_t* out, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, const SharpenParams& p,
                          hipStream_t stream);

// ---- producer passes (raster.hip) ----
struct crychic_pass_constants_viewproj { float m[16]; };   // one transposed 4x4 passed by value in the kernarg segment
struct Texture;
struct RasterPass {
    int mode;                               // 0 shadow depth, 1 view normals + depth, 2 G-buffer + depth, 3 normals + G-buffer + depth
    const float* view;                      // PassConstants.View (transposed storage)
    const float* viewProj;                  // PassConstants.ViewProj
    const crychic_draw_item* items; uint32_t nItems;     // host array, device pointers inside
    const crychic_material_data* materials; uint32_t nMaterials;   // device
    const Texture* textures; uint32_t nTextures;         // host array of {device pointer, w, h}
    uint32_t W, H;
    int depthBias; float slopeScaledDepthBias;
    uint32_t* depth; void* normal; float* g0; float* g1; float* g2;
    void* workspace; size_t workspaceBytes;
    uint32_t gRow0, gRows;                  // G-buffer rows to render (a rank's strip); gRows == 0 = the whole target
    uint32_t gbufferFlags;                  // CRYCHIC_GBUFFER_G*_F16: that plane's pointer (g0 / g1 / g2) addresses half4 texels
    const uint32_t* statusWord;             // OUT: device address of the pass's status word (bit 0: a vertex left the +-2^22 px
                                            // range and its triangle was dropped; bit 1: a vertex index outside the vertex buffer)
    // fused shadow pass (mode 0, nTargets 2..4): one ViewProj and one depth target per cascade, same items
    uint32_t nTargets; const float* viewProjN[4]; uint32_t* depthN[4];
};
size_t raster_workspace_bytes(uint64_t triangles, uint32_t W, uint32_t H);
hipError_t launch_raster_pass(RasterPass& p, hipStream_t stream);

}  // namespace cry
