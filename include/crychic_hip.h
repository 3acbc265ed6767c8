/*
 * crychic_hip.h -- C ABI of libcrychic_hip.so, the MI355X (gfx950) backend for CRYCHIC's per-pixel
 * hot path: G-buffer -> 14-tap SSAO -> bilateral blur -> deferred PBR lighting with cascaded-shadow PCF.
 *
 * The reference (UnlimitedRainWorks/CRYCHIC-RENDERER) has no FFI: the seam is the public surface of its
 * pass objects (Ssao.h:10-125, DeferredShading.h:4-45, ShadowMap.h:4-47), FrameResource.h and
 * CRYCHIC::Draw (CRYCHIC.cpp:172-306).  Every entry point below cites the reference code it replaces.
 * The C++ veneer in include/crychic/ keeps the reference's class and method names on top of this ABI.
 *
 * Conventions
 *   - plain pointers and sizes only; every `*_dev` pointer is DEVICE memory (hipMalloc or equivalent),
 *     every constant-buffer pointer is HOST memory and is copied at call time (the caller may reuse
 *     it immediately, like an UploadBuffer slot guarded by the frame fence, CRYCHIC.cpp:135-146);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     stream-ordered and asynchronous, there is no host synchronisation inside any entry point;
 *   - every function returns 0 on success or a negative crychic_status; crychic_last_error()
 *     returns a thread-local description (the reference throws DxException, Common/d3dUtil.h:132-144);
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails.
 *
 * Plane layouts (row-major, pitch = width * texel size, no tiling)
 *   depth    uint32  D24 in bits 0..23 (stencil bits ignored)           W x H
 *   normal   4 x fp16 view-space normal (DrawNormals.hlsl:93)            W x H
 *   ambient  uint16 R16_UNORM (Ssao.h:21)                                (W/2) x (H/2)
 *   randvec  4 x uint8 R8G8B8A8_UNORM (Ssao.cpp:362)                     256 x 256
 *   g0,g1,g2 4 x fp32 (GBuffer.hlsl:22-31)                               W x H
 *   shadow   uint32 D24 per cascade (ShadowMap.cpp:83,94)                shadowDim x shadowDim
 *   cube     4 x uint8 RGBA, faces +X,-X,+Y,-Y,+Z,-Z                     6 x cubeDim x cubeDim
 *   out      4 x uint8 R8G8B8A8_UNORM back buffer (Common/d3dApp.h:124)  W x H
 *   edge     opaque half-res workspace, crychic_edge_plane_bytes(W,H) bytes (see crychic_ssao)
 * W and H must be even (the half-res maps are W/2 x H/2, Ssao.cpp:22-30); the smallest frame is 2 x 2, the largest 2^28 pixels
 * with W < 2^20 and H <= 262140 (CRYCHIC_E_UNSUPPORTED beyond).
 */
#ifndef CRYCHIC_HIP_H
#define CRYCHIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRYCHIC_MAX_LIGHTS 16 /* Common/d3dUtil.h:226 */

typedef enum crychic_status {
    CRYCHIC_OK = 0,
    CRYCHIC_E_INVALID_ARG = -1,   /* null pointer, odd/zero size, bad range */
    CRYCHIC_E_NO_DEVICE = -2,     /* no HIP device / wrong ordinal */
    CRYCHIC_E_HIP = -3,           /* a HIP runtime call failed (see crychic_last_error) */
    CRYCHIC_E_UNSUPPORTED = -4,
    CRYCHIC_E_COMM = -5           /* RCCL failure */
} crychic_status;

/* Common/d3dUtil.h:216-224 (48 B) */
typedef struct crychic_light {
    float Strength[3];
    float FalloffStart;
    float Direction[3];
    float FalloffEnd;
    float Position[3];
    float SpotPower;
} crychic_light;

/* FrameResource.h:29-51 == cbPass Shaders/Common.hlsl:82-107 (2048 B).  Matrices are stored as the
 * reference stores them: XMMatrixTranspose of the row-vector matrix (CRYCHIC.cpp:843-849). */
typedef struct crychic_pass_constants {
    float View[16];
    float InvView[16];
    float Proj[16];
    float InvProj[16];
    float ViewProj[16];
    float InvViewProj[16];
    float ViewProjTex[16];
    float ShadowTransforms[12][16];
    float EyePosW[3];
    float cbPerObjectPad1;
    float RenderTargetSize[2];
    float InvRenderTargetSize[2];
    float NearZ;
    float FarZ;
    float TotalTime;
    float DeltaTime;
    float AmbientLight[4];
    crychic_light Lights[CRYCHIC_MAX_LIGHTS];
} crychic_pass_constants;

/* FrameResource.h:53-67 == cbSsao Shaders/Ssao.hlsl:5-22 (496 B) */
typedef struct crychic_ssao_constants {
    float Proj[16];
    float InvProj[16];
    float ProjTex[16];
    float OffsetVectors[14][4];
    float BlurWeights[3][4];
    float RenderTargetSize[2];
    float InvRenderTargetSize[2];
    float OcclusionRadius;
    float OcclusionFadeStart;
    float OcclusionFadeEnd;
    float SurfaceEpsilon;
} crychic_ssao_constants;

/* Camera state consumed by the constant builders (Common/Camera.h:20-97). */
typedef struct crychic_camera {
    float pos[3];
    float look[3];
    float up[3];
    float fovY, aspect, nearZ, farZ;
} crychic_camera;

typedef struct crychic_ctx crychic_ctx;

/* ---- context / errors ---------------------------------------------------------------------------- */
/* Replaces D3DApp::InitDirect3D's device creation (Common/d3dApp.cpp:415-479): binds the context to one
 * GPU.  One context per GPU, single-threaded, like the reference's one queue / one list. */
int crychic_ctx_create(int device_ordinal, crychic_ctx** out);
void crychic_ctx_destroy(crychic_ctx* ctx);
const char* crychic_last_error(void);
const char* crychic_version(void);
/* Name of the device the context is bound to ("gfx950..."); NULL on error. */
const char* crychic_ctx_device_name(crychic_ctx* ctx);

/* ---- host-side constant builders (no GPU needed) --------------------------------------------------- */
/* Ssao::CalcGaussWeights  Ssao.cpp:37-68.  Returns the number of weights written (2*ceil(2*sigma)+1) or a
 * negative status if capacity is too small / radius > Ssao::MaxBlurRadius (the reference asserts). */
int crychic_calc_gauss_weights(float sigma, float* weights, int capacity);
/* MathHelper::RandF over the MSVC CRT rand() LCG the reference links against (Common/MathHelper.h:17-20). */
int crychic_msvc_rand(uint32_t* state);
/* Ssao::BuildOffsetVectors  Ssao.cpp:423-462 */
void crychic_build_offset_vectors(uint32_t* rand_state, float offsets[14][4]);
/* Ssao::BuildRandomVectorTexture  Ssao.cpp:392-402 (texel bytes as the shader samples them). */
void crychic_build_random_vector_texture(uint32_t* rand_state, int args_right_to_left, uint8_t* rgba8_256x256);
/* CRYCHIC::UpdateCascadeShadowTransform  CRYCHIC.cpp:634-815.  Outputs are the untransposed row-vector
 * matrices (mLightViews / mLightProjs / mShadowTransforms). */
int crychic_update_cascade_shadow_transform(const crychic_camera* cam, const float lightDir[3],
                                            uint32_t shadowMapWidth, float lightView[4][16],
                                            float lightProj[4][16], float shadowTransform[4][16]);
/* CRYCHIC::UpdateMainPassCB  CRYCHIC.cpp:817-868 */
int crychic_update_main_pass_cb(const crychic_camera* cam, uint32_t W, uint32_t H,
                                const float shadowTransform[4][16], const float lightDirs[3][3],
                                crychic_pass_constants* out);
/* CRYCHIC::UpdateSsaoCB  CRYCHIC.cpp:903-937 */
int crychic_update_ssao_cb(const crychic_camera* cam, uint32_t W, uint32_t H, const float offsets[14][4],
                           crychic_ssao_constants* out);
/* Common.hlsl:305 `5 / width / 2.0f`.  literal != 0 keeps the shader's unsigned integer division (radius 0
 * for every width > 5: what the reference computes); literal == 0 gives the float division (2.5 texels). */
float crychic_pcf_search_radius(uint32_t shadowMapWidth, int literal);

/* ---- SSAO (Ssao.h / Ssao.cpp / Ssao.hlsl / SsaoBlur.hlsl) --------------------------------------------- */
/* Bytes of the edge workspace for a W x H frame: per-pixel centre normals / linear depths and recorded blur decisions (half
 * res), the decoded depth-pairs plane (full res) and the coarse maps of the exact shortcuts (csrc/ssao_core.hpp).
 * Contract: the workspace is caller-owned scratch with NO initialisation requirement and no meaning between frames -- it may
 * be freshly allocated, recycled from another context, or shared by consecutive frames of one stream.  Every word a frame
 * reads was written earlier in that same frame (the maps are stamped from one process-wide counter and the passes write the
 * stamp or a non-stamp into every word they will look at), so stale contents can never be mistaken for this frame's.  Parts
 * of it are deliberately left unwritten (depth-pairs entries under clear sky, which nothing reads): do not read it back. */
size_t crychic_edge_plane_bytes(uint32_t W, uint32_t H);

/* Ssao.hlsl:PS (Shaders/Ssao.hlsl:117-199) over half-res rows [row0, row0+rows): writes ambient_out and,
 * when edge_dev is not NULL, the per-pixel centre normal / linear depth that every later blur sweep of
 * this frame re-uses (SsaoBlur.hlsl:109-111,121-123 recompute them per tap). */
int crychic_ssao(crychic_ctx* ctx, const crychic_ssao_constants* cb, const void* normal_dev,
                 const uint32_t* depth_dev, const uint8_t* randvec_dev, uint16_t* ambient_out_dev,
                 void* edge_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows, void* stream);

/* Builds only the edge workspace (for callers that blur an ambient map they produced elsewhere). */
int crychic_ssao_edges(crychic_ctx* ctx, const crychic_ssao_constants* cb, const void* normal_dev,
                       const uint32_t* depth_dev, void* edge_dev, uint32_t W, uint32_t H, uint32_t row0,
                       uint32_t rows, void* stream);

/* One sweep of SsaoBlur.hlsl:PS == Ssao::BlurAmbientMap(cmdList, bool horzBlur) (Ssao.cpp:245-293) over
 * half-res rows [row0, row0+rows).  `horizontal` is the gHorizontalBlur root constant. */
int crychic_ssao_blur(crychic_ctx* ctx, const crychic_ssao_constants* cb, const void* edge_dev,
                      const uint16_t* ambient_in_dev, uint16_t* ambient_out_dev, uint32_t W, uint32_t H,
                      int horizontal, uint32_t row0, uint32_t rows, void* stream);

/* Ssao::ComputeSsao(cmdList, currFrame, blurCount)  Ssao.cpp:185-243: SSAO into ambient0, then blurCount x
 * (H: 0->1, V: 1->0); the final AO is in ambient0 (Ssao.cpp:75-78).  Rows [row0, row0+rows) of the final
 * map are guaranteed valid; the implementation recomputes a halo of 5 rows per remaining vertical sweep
 * (multi-GPU strips need no exchange).  row0 = 0, rows = H/2 is the whole map. */
int crychic_ssao_compute(crychic_ctx* ctx, const crychic_ssao_constants* cb, const void* normal_dev,
                         const uint32_t* depth_dev, const uint8_t* randvec_dev, uint16_t* ambient0_dev,
                         uint16_t* ambient1_dev, void* edge_dev, uint32_t W, uint32_t H, int blurCount,
                         uint32_t row0, uint32_t rows, void* stream);

/* ---- deferred lighting (DeferredShading.hlsl:PS, Shaders/DeferredShading.hlsl:23-101) ------------------ */
#define CRYCHIC_LIGHT_SKY 1u /* fill uncovered pixels from the cubemap (sky.hlsl:21-47) instead of the clear colour */
/* The reference's shader quirks are reproduced by default (SURVEY.md quirk checklist); each switch selects the evidently
 * intended form instead, for callers that want the fixed maths (parity is then against this repo's oracle with the same flag):
 *   Q1  DeferredShading.hlsl:60 `abs(distance - radius[j] < 5.0f)` (abs of a bool: always blends cascades j and j+1)
 *       -> `abs(distance - radius[j]) < 5.0f`, the form of the forward shader (Default.hlsl:131)
 *   Q3  PBR.hlsl:58,66 the specular denominator uses hDotv where nDotv is meant -> nDotl * nDotv
 *   Q4  PBR.hlsl:61-68 `ks * fs` with fs already holding F (Fresnel applied twice) -> kd * fd + fs */
/* The cube map's mip chain (the reference binds the whole chain, CRYCHIC.cpp:1148-1151, and samples it MIN_MAG_MIP_LINEAR,
 * :2617-2622): CRYCHIC_LIGHT_CUBE_LEVELS(n) in `flags` says that cube_dev holds n levels (crychic_load_dds_cube_rgba8_mips' layout:
 * level after level, each six faces of max(cubeDim >> level, 1)^2 RGBA8 texels); the reflection lookup (DeferredShading.hlsl:95)
 * and the sky (sky.hlsl:46) are then trilinear, the level of detail taken from the direction's differences inside the pixel's
 * 2 x 2 quad -- a BUILD DEFINITION (D3D leaves the arithmetic to the hardware; DESIGN.md section 3 states it), parity against
 * this repo's CPU checker.  n = 0 or 1: level 0 alone, the lookup of every earlier release.  With n > 1 a call's rows must be whole
 * quad rows (even row0; even rows unless they end the frame). */
#define CRYCHIC_LIGHT_CUBE_LEVELS(n) (((uint32_t)(n) & 15u) << 16)
/* Glossy reflections (BUILD-DEFINED EXTENSION).  CRYCHIC_LIGHT_CUBE_GLOSS, valid only together with
 * CRYCHIC_LIGHT_CUBE_LEVELS(n), n > 1 (otherwise CRYCHIC_E_INVALID_ARG), says that cube_dev holds a chain prefiltered by roughness
 * (crychic_prefilter_cube_chain below): the reflection lookup of DeferredShading.hlsl:95 is then trilinear at
 * lod = saturate(roughness) * (n - 1) -- one multiply; roughness is the decoded G-buffer value the pixel's BRDF uses, NaN -> 0 --
 * instead of the quad's derivatives; `shininess` and the Fresnel factor of :96-97 stay as written.  The sky reads level 0 alone,
 * as without a chain.  No quad is involved, so the rows of a call need not be whole quad rows.  Accepted by every
 * crychic_deferred_light* entry and in crychic_frame_desc.flags; without the flag every call is what it was, bit for bit. */
#define CRYCHIC_LIGHT_CUBE_GLOSS 0x800u
/* Ambient light from the cube map (BUILD-DEFINED EXTENSION; "SH9 irradiance" below).  With
 * CRYCHIC_LIGHT_AMBIENT_SH the ambient term of DeferredShading.hlsl:44 takes its colour from the nine order-2 spherical-harmonics
 * coefficients that follow the cube map in memory -- cube_dev + crychic_cube_sh_offset(cubeDim, levels) holds the environment tail --
 * instead of AmbientLight, which is not read.  Valid with no chain (CRYCHIC_LIGHT_CUBE_LEVELS 0 or 1) and with
 * CRYCHIC_LIGHT_CUBE_LEVELS(n > 1) | CRYCHIC_LIGHT_CUBE_GLOSS; with the derivative-LOD chain (n > 1 without gloss)
 * CRYCHIC_E_UNSUPPORTED.  A tail that is not 4-byte aligned is CRYCHIC_E_INVALID_ARG, before anything is enqueued.  Accepted by every
 * crychic_deferred_light* entry and in crychic_frame_desc.flags; without the flag every call is what it was, bit for bit. */
#define CRYCHIC_LIGHT_AMBIENT_SH 0x8000u
/* Split-sum specular from the environment (BUILD-DEFINED EXTENSION; "environment BRDF table" below).  With
 * CRYCHIC_LIGHT_ENV_BRDF the reflection term of DeferredShading.hlsl:97 is weighed by the second factor of the split sum, filtered from
 * the 32 x 32 table that follows the environment tail in memory -- cube_dev + crychic_cube_env_brdf_offset(cubeDim, levels) holds the
 * table -- instead of shininess * SchlickFresnel(R0, normalW, r), which are not evaluated.  Valid only together with
 * CRYCHIC_LIGHT_CUBE_LEVELS(n > 1) | CRYCHIC_LIGHT_CUBE_GLOSS, with and without CRYCHIC_LIGHT_AMBIENT_SH (the 512-byte tail before the
 * table is read only under that flag); anything else, a NULL cube map or a table address that is not 4-byte aligned is
 * CRYCHIC_E_INVALID_ARG with a message, before anything is enqueued.  Accepted by every crychic_deferred_light* entry (strips and the
 * _shared entries included) and in crychic_frame_desc.flags; without the flag every call is what it was, bit for bit. */
#define CRYCHIC_LIGHT_ENV_BRDF 0x100000u
/* Parallax-corrected reflections (BUILD-DEFINED EXTENSION; "probe volume" below).  With
 * CRYCHIC_LIGHT_CUBE_PARALLAX the reflection lookup of DeferredShading.hlsl:95 takes, in place of the reflection vector, the direction
 * from the capture position to the point where the reflection ray from the pixel's own world position leaves the probe volume's box
 * -- the twelve floats at cube_dev + crychic_cube_probe_offset(cubeDim, levels), inside the environment tail.  Valid only together with
 * CRYCHIC_LIGHT_CUBE_LEVELS(n > 1) | CRYCHIC_LIGHT_CUBE_GLOSS, with and without CRYCHIC_LIGHT_AMBIENT_SH and CRYCHIC_LIGHT_ENV_BRDF and
 * with any G-buffer format mix; any other combination, a NULL cube map or a probe volume address that is not 4-byte aligned is
 * CRYCHIC_E_INVALID_ARG with a message, before anything is enqueued.  Accepted by every crychic_deferred_light* entry (strips and the
 * _shared entries included) and in crychic_frame_desc.flags; without the flag every call is what it was, bit for bit. */
#define CRYCHIC_LIGHT_CUBE_PARALLAX 0x200000u
#define CRYCHIC_FIX_Q1 0x100u
#define CRYCHIC_FIX_Q3 0x200u
#define CRYCHIC_FIX_Q4 0x400u
/* The G-buffer plane formats.  Each of G0, G1 and G2 is, independently, float4 texels (16 bytes, the default) or
 * half4 texels (8 bytes: IEEE binary16, x in the low half of the first dword -- DXGI_FORMAT_R16G16B16A16_FLOAT, the normal map's
 * layout).  A set bit in `flags` (every crychic_deferred_light* entry, crychic_frame_desc.flags, crychic_draw_gbuffer_formats) says that
 * the plane's pointer addresses half4 texels; the `const float*` / `float*` parameters keep their type and the caller casts.  All
 * eight combinations are valid, flags without these bits is every earlier release's call.
 * The format is STORAGE ONLY.  Write (producers): the fp32 value the pass computes is rounded to nearest even, subnormals kept,
 * overflow (|x| > 65504 after rounding) to infinity -- the render-target conversion of the normal map; the clear value is all-zero
 * bits.  Read (lighting): the texel widens exactly, and everything after the load is the fp32 arithmetic of the float4 path; there
 * is no fp16 arithmetic anywhere.  So: light(planes in any mix) == light(those planes widened to float4) bit for bit, and
 * producer(mix) == round_to_half(producer's float4 planes) bit for bit on the half planes, the other outputs unchanged.
 * fp16 WORLD POSITIONS ARE COARSE: G0.xyz has an ulp of 1/64 unit at 16..32 units from the origin (1/8 at 128..256), which is what
 * the format means in D3D too.  G0 float4 with G1 + G2 half4 (32 bytes per pixel instead of 48) is the practical mix; all three half4
 * (24 bytes) is what DeferredShading(..., DXGI_FORMAT_R16G16B16A16_FLOAT) means. */
#define CRYCHIC_GBUFFER_G0_F16 0x1000u
#define CRYCHIC_GBUFFER_G1_F16 0x2000u
#define CRYCHIC_GBUFFER_G2_F16 0x4000u
#define CRYCHIC_GBUFFER_F16_MASK 0x7000u
/* Bytes of plane `plane` (0, 1, 2 = G0, G1, G2) of a W x H G-buffer under `flags` (their CRYCHIC_GBUFFER_* bits); 0 for any other
 * plane index.  Pure host arithmetic. */
size_t crychic_gbuffer_plane_bytes(uint32_t W, uint32_t H, uint32_t flags, int plane);

/* Full-screen replacement of the geometry re-draw at CRYCHIC.cpp:238-273 over full-res rows
 * [row0, row0+rows): pixels with depth < 1.0 are lit, the others get Colors::LightSteelBlue
 * (CRYCHIC.cpp:247) or the sky.  ambient_dev may be NULL (SSAO off, ambientAccess = 1); radiance_out_dev
 * (optional, 4 floats per pixel) receives litColor before UNORM8 quantisation.  numDirLights is the
 * shader's NUM_DIR_LIGHTS (1 in the reference build, Common.hlsl:6-8). */
int crychic_deferred_light(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev,
                           const float* g1_dev, const float* g2_dev, const uint32_t* depth_dev,
                           const uint16_t* ambient_dev, const uint32_t* const shadow_dev[4], uint32_t shadowDim,
                           const uint8_t* cube_dev, uint32_t cubeDim, uint8_t* out_rgba8_dev,
                           float* radiance_out_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                           int numDirLights, float pcfSearchRadius, uint32_t flags, void* stream);

/* crychic_deferred_light plus `numPointLights` (<= 1024) point lights read from a device array of crychic_light
 * (Strength, FalloffStart, FalloffEnd, Position).  BUILD-DEFINED EXTENSION: the reference's NUM_POINT_LIGHTS branch
 * (PBR.hlsl:109-124) is dead code; it is enabled here as evidently intended (range test, l /= d, linear attenuation,
 * shadow factor 1) with per-tile light culling in LDS.  Parity is against this repo's oracle only. */
int crychic_deferred_light_points(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev,
                                  const float* g1_dev, const float* g2_dev, const uint32_t* depth_dev,
                                  const uint16_t* ambient_dev, const uint32_t* const shadow_dev[4], uint32_t shadowDim,
                                  const uint8_t* cube_dev, uint32_t cubeDim, uint8_t* out_rgba8_dev,
                                  float* radiance_out_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                                  int numDirLights, float pcfSearchRadius, uint32_t flags,
                                  const crychic_light* point_lights_dev, uint32_t numPointLights, void* stream);

/* crychic_deferred_light_points plus `numSpotLights` (<= 1024) spot lights read from a second device array of crychic_light
 * (all six fields).  BUILD-DEFINED EXTENSION like the point lights: the reference's NUM_SPOT_LIGHTS branch (PBR.hlsl:126-147)
 * is dead code; parity is against this repo's checker only.  Definition -- after the directional and the point lights, spot
 * lights in ascending index order (the gLights order, Common.hlsl:102-105), each one:
 *   l = Position - pos;  d = |l|;  d > FalloffEnd: no contribution;  l *= rcp(d);
 *   att = saturate((FalloffEnd - d) / (FalloffEnd - FalloffStart));
 *   att = att * pow(max(dot(-Direction, l), 0.001), SpotPower)     (one rounding; pow = exp2(clamp(y * log2 x, -125, 127)))
 *   lightStrength = Strength * nDotl * att;  result = fma(brdf, lightStrength, result)   (shadow factor 1)
 * with the point lights' BRDF (CRYCHIC_FIX_Q3 / Q4 included).  Direction is used as given (not normalised).  SpotPower = 0
 * gives a factor of exactly 1, i.e. the bits of a point light at the same position.  The 0.001 floor means a spot light never
 * contributes exactly zero outside its cone, so tiles cull spot lights by their range sphere alone, exactly as point lights.
 * numSpotLights == 0 is crychic_deferred_light_points, bit for bit.  numSpotLights > 1024, or a NULL spot_lights_dev with
 * numSpotLights > 0, returns CRYCHIC_E_INVALID_ARG. */
int crychic_deferred_light_spots(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev,
                                 const float* g1_dev, const float* g2_dev, const uint32_t* depth_dev,
                                 const uint16_t* ambient_dev, const uint32_t* const shadow_dev[4], uint32_t shadowDim,
                                 const uint8_t* cube_dev, uint32_t cubeDim, uint8_t* out_rgba8_dev,
                                 float* radiance_out_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                                 int numDirLights, float pcfSearchRadius, uint32_t flags,
                                 const crychic_light* point_lights_dev, uint32_t numPointLights,
                                 const crychic_light* spot_lights_dev, uint32_t numSpotLights, void* stream);

/* ---- shadowed spot lights (BUILD-DEFINED EXTENSION; parity against this repo's checker, tests/local_light_ref) --------- *
 * The reference declares gShadowMap[12] / gShadowTransforms[12] (Common.hlsl:46,91), of which the cascades use slots 0..3, and
 * leaves the spot branch's `result += shadowFactor[i] * brdf * lightStrength` commented out (PBR.hlsl:145).  Here the first
 * `count` (<= CRYCHIC_MAX_SPOT_SHADOWS) spot lights fill slots 4..11: spot light k < count reads
 *   maps[k]: D24 in the low 24 bits of a uint32, square, side `dim` (the cascades' format), sampled with gsamShadow
 *            (LESS_EQUAL, border 0);
 *   passCB->ShadowTransforms[4 + k]: stored transposed like the cascade transforms (crychic_update_spot_shadow_transform).
 * Spot lights k >= count keep shadow factor 1.  Shadow factor s -- CalcShadowFactor (Common.hlsl:135-165) with its hard-wired
 * gShadowMap[0] generalised to the light's own map:
 *   sp = mul(float4(posW, 1), T);  rw = rcp(sp.w);  x = sp.x * rw;  y = sp.y * rw;  depth = sp.z * rw   (as the cascades' PCF)
 *   dx = 1.0f / (float)dim   (correctly rounded)
 *   nine taps in the order of offsets[9] (:150-155: y outer, x inner, offsets -dx, 0, +dx), each
 *       gsamShadow.SampleCmpLevelZero(map, float2(x + ox, y + oy), depth)   (each coordinate one float add, not an fma)
 *   summed in that order from 0.0f;  s = percentLit / 9.0f   (correctly rounded)
 * Non-finite coordinates address only border texels and give 0; positions behind the light (sp.w <= 0) are taken literally
 * (no w == 1 shortcut: the transforms are perspective).  The spot term becomes result = fma(s * brdf, lightStrength, result):
 * s == 1 gives the unshadowed bits, s == 0 leaves result unchanged for finite inputs.  s is evaluated only where the spot term
 * is (d <= FalloffEnd); the tile cull stays spherical.
 * A NULL descriptor or count == 0 is the matching _spots entry, bit for bit.  With count > 0: count > 8, count > numSpotLights,
 * a NULL map among the first count, dim < 2 or dim > CRYCHIC_MAX_SPOT_SHADOW_DIM return CRYCHIC_E_INVALID_ARG (with a message)
 * before anything is enqueued.  The maps are rendered by crychic_draw_scene_to_shadow_maps with passCBs[k].ViewProj = V * P of
 * crychic_update_spot_shadow_transform. */
#define CRYCHIC_MAX_SPOT_SHADOWS 8
#define CRYCHIC_MAX_SPOT_SHADOW_DIM 16384
typedef struct crychic_spot_shadows {
    uint32_t count;
    uint32_t dim;
    const uint32_t* maps[CRYCHIC_MAX_SPOT_SHADOWS];
} crychic_spot_shadows;

/* crychic_deferred_light_spots with the first spotShadows->count spot lights shadowed (definition above). */
int crychic_deferred_light_spots_shadowed(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev,
                                          const float* g1_dev, const float* g2_dev, const uint32_t* depth_dev,
                                          const uint16_t* ambient_dev, const uint32_t* const shadow_dev[4], uint32_t shadowDim,
                                          const uint8_t* cube_dev, uint32_t cubeDim, uint8_t* out_rgba8_dev,
                                          float* radiance_out_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                                          int numDirLights, float pcfSearchRadius, uint32_t flags,
                                          const crychic_light* point_lights_dev, uint32_t numPointLights,
                                          const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                          const crychic_spot_shadows* spotShadows, void* stream);

/* The light, projection and shadow transform of a shadowed spot light (host only; the counterpart of
 * crychic_update_cascade_shadow_transform, whose storage it follows: untransposed row-vector matrices, copied TRANSPOSED
 * into passCB->ShadowTransforms[4 + k]):
 *   lightView = LookAtLH(Position, Position + Direction, up), up = (0, 1, 0), or (0, 0, 1) when
 *               |dot(Direction, (0, 1, 0))| > 0.999 |Direction| (a light aimed straight up or down);
 *   lightProj = PerspectiveFovLH(fovY, 1, zNear, FalloffEnd);
 *   shadowTransform = lightView * lightProj * T, T the NDC -> texture matrix of the cascades (CRYCHIC.cpp:804-813).
 * The shadow pass renders with ViewProj = lightView * lightProj.  CRYCHIC_E_INVALID_ARG for a NULL pointer, a zero Direction,
 * fovY outside (0, pi), zNear <= 0 or zNear >= FalloffEnd. */
int crychic_update_spot_shadow_transform(const crychic_light* L, float fovY, float zNear, float lightView[16], float lightProj[16],
                                         float shadowTransform[16]);

/* ---- shadowed point lights (BUILD-DEFINED EXTENSION; parity against this repo's checker, tests/point_shadow_ref) ---------- *
 * Omnidirectional (cube) shadows for the first `count` (<= CRYCHIC_MAX_POINT_SHADOWS) point lights.  Point light k < count reads
 * six dim x dim D24 faces stored back to back at maps[k] (+X, -X, +Y, -Y, +Z, -Z; the spot maps' format) through one projection
 * shadowProj[k] (untransposed, as crychic_update_point_shadow_transforms writes it).  Where the point term is evaluated
 * (d <= FalloffEnd; the tile cull stays spherical):
 *   v = pos - Position                                    (three float subtractions: -l of the point term)
 *   ax, ay, az = |v|;  face axis X if ax >= ay && ax >= az, else Y if ay >= az, else Z;  positive when that component >= 0.0f
 *   face view coordinates (a, b, c), exact sign flips and permutations of v (LookAtLH(Position, Position + axis, up)):
 *     +X (-v.z, v.y, v.x)   -X (v.z, v.y, -v.x)   +Y (v.x, -v.z, v.y)   -Y (v.x, v.z, -v.y)   +Z (v.x, v.y, v.z)   -Z (-v.x, v.y, -v.z)
 *     up = (0, 1, 0) for +-X and +-Z, (0, 0, -1) for +Y, (0, 0, 1) for -Y
 *   s = the spot lights' 9-tap factor (crychic_deferred_light_spots_shadowed) on face f of maps[k] with T = shadowProj[k]
 *       transposed, at the position (a, b, c): perspective divide, nine gsamShadow taps in offsets[9] order, / 9.0f
 *   result = fma(s * brdf, lightStrength, result)         (s == 1: the unshadowed bits)
 * Point lights k >= count keep shadow factor 1.  crychic_update_point_shadow_transforms widens each face so that every point of
 * its 90-degree region lands at texel coordinates in [2, dim - 2]: all nine taps' footprints stay inside the face (no seams).
 * A NULL descriptor or count == 0 is the matching _spots_shadowed entry, bit for bit.  With count > 0: count > 4,
 * count > numPointLights, a NULL map among the first count, dim < 16 or dim > CRYCHIC_MAX_SPOT_SHADOW_DIM return
 * CRYCHIC_E_INVALID_ARG (with a message) before anything is enqueued.  Face f is rendered by crychic_draw_scene_to_shadow_maps
 * with passCBs[i].ViewProj = lightView[f] * lightProj (the cascades' bias, 10000 / 2.0; at most 12 faces, two lights, per call). */
#define CRYCHIC_MAX_POINT_SHADOWS 4
#define CRYCHIC_MIN_POINT_SHADOW_DIM 16            /* max: CRYCHIC_MAX_SPOT_SHADOW_DIM */
typedef struct crychic_point_shadows {
    uint32_t count;                                 /* point lights 0 .. count-1 are shadowed */
    uint32_t dim;                                   /* face side */
    const uint32_t* maps[CRYCHIC_MAX_POINT_SHADOWS];  /* six dim x dim D24 faces back to back: +X, -X, +Y, -Y, +Z, -Z */
    float shadowProj[CRYCHIC_MAX_POINT_SHADOWS][16];  /* as crychic_update_point_shadow_transforms writes it (untransposed) */
} crychic_point_shadows;

/* crychic_deferred_light_spots_shadowed with the first pointShadows->count point lights shadowed (definition above). */
int crychic_deferred_light_point_shadows(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev,
                                         const float* g1_dev, const float* g2_dev, const uint32_t* depth_dev,
                                         const uint16_t* ambient_dev, const uint32_t* const shadow_dev[4], uint32_t shadowDim,
                                         const uint8_t* cube_dev, uint32_t cubeDim, uint8_t* out_rgba8_dev,
                                         float* radiance_out_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                                         int numDirLights, float pcfSearchRadius, uint32_t flags,
                                         const crychic_light* point_lights_dev, uint32_t numPointLights,
                                         const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                         const crychic_spot_shadows* spotShadows, const crychic_point_shadows* pointShadows,
                                         void* stream);

/* The six face views, the projection and the shadow projection of a shadowed point light (host only; the storage of
 * crychic_update_spot_shadow_transform: untransposed row-vector matrices):
 *   lightView[f] = LookAtLH(Position, Position + axis_f, up_f)   (the face table above; entries exactly 0, +-1 and -dot(axis, Position))
 *   lightProj    = PerspectiveFovLH with aspect 1, zNear .. FalloffEnd and xScale = yScale = (dim - 4) / dim
 *                  (fovY = 2 atan(dim / (dim - 4)): the widened face)
 *   shadowProj   = lightProj * T, T the NDC -> texture matrix of the cascades; the descriptor's shadowProj[k].
 * The shadow pass of face f renders with ViewProj = lightView[f] * lightProj.  CRYCHIC_E_INVALID_ARG for a NULL pointer, dim
 * outside 16 .. 16384, zNear <= 0, zNear >= FalloffEnd or a non-finite Position. */
int crychic_update_point_shadow_transforms(const crychic_light* L, uint32_t dim, float zNear, float lightView[6][16],
                                           float lightProj[16], float shadowProj[16]);

/* ---- whole hot path of CRYCHIC::Draw (CRYCHIC.cpp:220-221 + 238-279) -------------------------------------- */
typedef struct crychic_frame_desc {
    uint32_t W, H;
    int blurCount;              /* CRYCHIC.cpp:221 passes 3; <0 = SSAO off */
    int numDirLights;
    float pcfSearchRadius;
    uint32_t flags;             /* CRYCHIC_LIGHT_* */
    uint32_t row0, rows;        /* full-res output rows owned by this GPU (0, H = whole frame) */
    const void* normal_dev;
    const uint32_t* depth_dev;
    const uint8_t* randvec_dev;
    const float* g0_dev;
    const float* g1_dev;
    const float* g2_dev;
    const uint32_t* shadow_dev[4];
    uint32_t shadowDim;
    const uint8_t* cube_dev;
    uint32_t cubeDim;
    uint16_t* ambient0_dev;
    uint16_t* ambient1_dev;
    void* edge_dev;
    uint8_t* out_rgba8_dev;
    /* Extension (BASELINE configs[4], parity vs this repo's oracle only): point lights evaluated after the directional
     * ones, with tiled light culling; NULL / 0 = the reference configuration. */
    const crychic_light* point_lights_dev;
    uint32_t numPointLights;
} crychic_frame_desc;

int crychic_draw_hot_path(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB,
                          const crychic_pass_constants* passCB, const crychic_frame_desc* frame, void* stream);
/* crychic_draw_hot_path with `numSpotLights` spot lights after the frame's point lights (crychic_deferred_light_spots' definition
 * and limits); numSpotLights == 0 is crychic_draw_hot_path, bit for bit. */
int crychic_draw_hot_path_spots(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                                const crychic_frame_desc* frame, const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                void* stream);
/* crychic_draw_hot_path_spots with shadowed spot lights (crychic_deferred_light_spots_shadowed's definition and limits); a NULL
 * descriptor or count == 0 is crychic_draw_hot_path_spots, bit for bit. */
int crychic_draw_hot_path_spots_shadowed(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                                         const crychic_frame_desc* frame, const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                         const crychic_spot_shadows* spotShadows, void* stream);
/* crychic_draw_hot_path_spots_shadowed with shadowed point lights (crychic_deferred_light_point_shadows' definition and limits);
 * a NULL point descriptor or count == 0 is crychic_draw_hot_path_spots_shadowed, bit for bit. */
int crychic_draw_hot_path_point_shadows(crychic_ctx* ctx, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                                        const crychic_frame_desc* frame, const crychic_light* spot_lights_dev, uint32_t numSpotLights,
                                        const crychic_spot_shadows* spotShadows, const crychic_point_shadows* pointShadows,
                                        void* stream);

/* Per-kernel timing of the last crychic_draw_hot_path issued with profiling enabled (HIP events recorded
 * on the caller's stream around each pass).  Times are milliseconds; blocks until the events complete. */
typedef struct crychic_pass_times {
    float ssao_ms;
    float blur_ms;   /* all 2*blurCount sweeps */
    float light_ms;
    float total_ms;
} crychic_pass_times;
int crychic_ctx_set_profiling(crychic_ctx* ctx, int enabled);
int crychic_ctx_last_pass_times(crychic_ctx* ctx, crychic_pass_times* out);


/* ---- producer passes: the draws that fill the hot path's input planes ------------------------- */
/* FrameResource.h:69-75 (44 B; input layout CRYCHIC.cpp:1241-1247) */
typedef struct crychic_vertex { float Pos[3]; float Normal[3]; float TexC[2]; float TangentU[3]; } crychic_vertex;
/* FrameResource.h:7-15 (144 B); matrices stored transposed as UpdateInstanceData writes them (CRYCHIC.cpp:546-547) */
typedef struct crychic_instance_data { float World[16]; float TexTransform[16]; uint32_t MaterialIndex; uint32_t pad[3]; } crychic_instance_data;
/* FrameResource.h:17-27 (112 B); MatTransform stored transposed (CRYCHIC.cpp:582) */
typedef struct crychic_material_data {
    float DiffuseAlbedo[4]; float FresnelR0[3]; float Roughness; float MatTransform[16];
    uint32_t DiffuseMapIndex; uint32_t NormalMapIndex; float Metalness; uint32_t pad;
} crychic_material_data;
/* One DrawIndexedInstanced(IndexCount, InstanceCount, StartIndexLocation, BaseVertexLocation, 0) with its bound vertex,
 * index (R32_UINT) and instance buffers (CRYCHIC::DrawRenderItems, CRYCHIC.cpp:2438-2475).  All pointers are device. */
typedef struct crychic_draw_item {
    const crychic_vertex* vertices_dev; uint32_t vertexCount;
    const uint32_t* indices_dev; uint32_t indexCount; uint32_t startIndexLocation; int32_t baseVertexLocation;
    const crychic_instance_data* instances_dev; uint32_t instanceCount;
} crychic_draw_item;
/* An R8G8B8A8_UNORM texture of gTextureMaps[] (Common.hlsl:52); rgba8_dev may be NULL (white / flat normal).  mipLevels > 1:
 * the levels follow one another in memory, level k being max(1, width >> k) x max(1, height >> k) texels (what
 * crychic_load_dds_rgba8_mips returns), and the G-buffer pass samples it as gsamAnisotropicWrap does (anisotropic 8, trilinear;
 * the kernel D3D leaves open is defined in csrc/raster_core.hpp).  mipLevels 0 or 1: level 0 only, bilinear. */
typedef struct crychic_texture { const uint8_t* rgba8_dev; uint32_t width, height, mipLevels; } crychic_texture;

/* GeometryGenerator::CreateBox / CreateGrid (Common/GeometryGenerator.cpp:10-101, 551-614) and the Models/<name>.txt loader
 * of CRYCHIC::BuildSkullGeometry (CRYCHIC.cpp:1447-1557), host memory.  Call with NULL buffers to get the counts.
 * Return the vertex count, or a negative status. */
int crychic_create_box(float width, float height, float depth, uint32_t numSubdivisions, crychic_vertex* vertices,
                       uint32_t vertexCapacity, uint32_t* indices, uint32_t indexCapacity, uint32_t* indexCount);
int crychic_create_grid(float width, float depth, uint32_t m, uint32_t n, crychic_vertex* vertices, uint32_t vertexCapacity,
                        uint32_t* indices, uint32_t indexCapacity, uint32_t* indexCount);
int crychic_load_mesh_text(const char* path, crychic_vertex* vertices, uint32_t vertexCapacity, uint32_t* indices,
                           uint32_t indexCapacity, uint32_t* vertexCount, uint32_t* indexCount);

/* CRYCHIC::UpdateInstanceData's frustum culling (CRYCHIC.cpp:515-564; mFrustumCullingEnabled defaults to true,
 * CRYCHIC.h:188): visible[i] = 1 when the render item's local-space bounding box (center, extents) under world matrix
 * worlds[16 i ..] (row-major, row-vector convention, untransposed) is not DISJOINT from the camera frustum.  Only visible
 * instances are copied to the frame's instance buffer, so a culled instance is also missing from the shadow pass.
 * Returns the number of visible instances (>= 0) or a negative status. */
int crychic_frustum_cull(const crychic_camera* cam, const float boundsCenter[3], const float boundsExtents[3],
                         const float* worlds, uint32_t count, uint8_t* visible);

/* Material textures: a DDS file holding DXT1, DXT5 or 32-bit-mask pixels (the formats of the six
 * textures CRYCHIC::LoadTextures opens, CRYCHIC.cpp:939-973) decoded on the host to the R8G8B8A8 mip-0 image that
 * crychic_draw_gbuffer samples.  NULL buffer: only *width / *height are written.  Replaces the subset of
 * Common/DDSTextureLoader.cpp + GPU block decompression the path depends on. */
int crychic_load_dds_rgba8(const char* path, uint8_t* rgba8, size_t capacityBytes, uint32_t* width, uint32_t* height);
/* The same with the file's whole mip chain (Common/DDSTextureLoader.cpp uploads the stored levels, it generates none): the
 * levels are written back to back, level k = max(1, w >> k) x max(1, h >> k); *mipLevels = the number of levels decoded.
 * NULL buffer: only the sizes are written; the bytes needed are the sum over the levels of 4 * w_k * h_k. */
int crychic_load_dds_rgba8_mips(const char* path, uint8_t* rgba8, size_t capacityBytes, uint32_t* width, uint32_t* height,
                                uint32_t* mipLevels);

/* The sky cube map CRYCHIC::LoadTextures opens (CRYCHIC.cpp:960,968: snowcube1024.dds through CreateDDSTextureFromFile12; bound
 * as a TextureCube, CRYCHIC.cpp:1148-1151): a DDS cube map -- DDSCAPS2_CUBEMAP with all six faces, or a DX10 header with
 * DDS_RESOURCE_MISC_TEXTURECUBE -- holding DXT1 / DXT5 / 32-bit pixels, decoded to the 6 x dim x dim R8G8B8A8 plane (faces +X, -X,
 * +Y, -Y, +Z, -Z stacked) that crychic_deferred_light / crychic_draw_hot_path take as the cube map.  Level 0 of every face: the
 * lighting and sky passes filter level 0.  NULL buffer: only *dim is written.  The 2-D loaders above refuse
 * a cube file and this one refuses a 2-D file (CRYCHIC_E_UNSUPPORTED). */
int crychic_load_dds_cube_rgba8(const char* path, uint8_t* rgba8, size_t capacityBytes, uint32_t* dim);
/* The same with the mip chain the file stores (CRYCHIC.cpp:1148-1151 binds every level): level after level, each level the six
 * faces of max(dim >> level, 1)^2 texels -- what CRYCHIC_LIGHT_CUBE_LEVELS(*mipLevels) announces to the lighting pass.  rgba8 = NULL
 * queries *dim and *mipLevels (capacity: sum over the levels of 6 * d * d * 4 bytes). */
int crychic_load_dds_cube_rgba8_mips(const char* path, uint8_t* rgba8, size_t capacityBytes, uint32_t* dim, uint32_t* mipLevels);

/* Present stand-in (row f3; the reference calls IDXGISwapChain::Present, CRYCHIC.cpp:294-297): writes a HOST R8G8B8A8
 * image as binary PPM (alpha dropped). */
int crychic_save_ppm(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);

/* Device workspace for one rasterised pass over `triangles` input triangles (sum over items of instanceCount *
 * indexCount / 3) into a W x H target: 8 bytes per target pixel plus SEVEN set-up slots (192 B + a 4-byte live word each)
 * per input triangle -- a triangle clipped against the six guard-band / depth planes becomes a fan of up to seven, and slots
 * are fixed by draw order so that depth ties resolve as D3D12 resolves them.  That is ~1.4 KB per triangle: ~450 MB for the
 * four fused 4096^2 cascades of the 81 k-triangle benchmark scene (4 x 81 k triangle-targets).  Only the slots a triangle
 * lists are written or read.  A workspace sized by a build older than the guard-band clipping (three slots per triangle) is
 * refused with CRYCHIC_E_INVALID_ARG, never overrun: always size it with this function of the library you link. */
size_t crychic_raster_workspace_bytes(uint64_t triangles, uint32_t W, uint32_t H);

/* The three producer passes.  Rasteriser state = CD3DX12_RASTERIZER_DESC(D3D12_DEFAULT): solid, cull back, clockwise
 * front, depth clip and guard-band clip (Common/d3dx12.h:203-216); depth LESS + write against a target cleared to 1.0 (:120-132);
 * top-left rule, pixel centres at +0.5, 1/256-pixel vertex snap.  `passCB` supplies View / ViewProj.  Every pass clears its
 * targets first, like the reference (CRYCHIC.cpp:2489-2492, 2526-2527, 2554-2556).
 *   crychic_draw_scene_to_shadow_map : one cascade of CRYCHIC::DrawSceneToShadowMap (CRYCHIC.cpp:2477-2510) with the
 *       shadow PSO's DepthBias / SlopeScaledDepthBias (CRYCHIC.cpp:1601-1603: 10000, 2.0)
 *   crychic_draw_normals_and_depth   : CRYCHIC::DrawNormalsAndDepth (CRYCHIC.cpp:2512-2543), DrawNormals.hlsl
 *   crychic_draw_gbuffer             : CRYCHIC::DrawGBuffer (CRYCHIC.cpp:2545-2571), GeometryPass.hlsl; depth_dev is
 *       the depth target of this pass (may alias the normals pass's: same geometry, same values) */
int crychic_draw_scene_to_shadow_map(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                                     uint32_t nItems, uint32_t* shadow_dev, uint32_t shadowDim, int depthBias,
                                     float slopeScaledDepthBias, void* workspace_dev, size_t workspaceBytes, void* stream);
int crychic_draw_normals_and_depth(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                                   uint32_t nItems, void* normal_dev, uint32_t* depth_dev, uint32_t W, uint32_t H,
                                   void* workspace_dev, size_t workspaceBytes, void* stream);
int crychic_draw_gbuffer(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                         uint32_t nItems, const crychic_material_data* materials_dev, uint32_t nMaterials,
                         const crychic_texture* textures, uint32_t nTextures, float* g0_dev, float* g1_dev, float* g2_dev,
                         uint32_t* depth_dev, uint32_t W, uint32_t H, void* workspace_dev, size_t workspaceBytes, void* stream);

/* What the most recent producer pass on this context could not draw (its workspace must still be alive): waits for `stream`, then
 * *flags = CRYCHIC_RASTER_* bits, 0 when every triangle was rasterised.  Triangles with vertices far outside the viewport ARE
 * drawn: like the D3D12 runtime the rasteriser clips to 0 <= z <= w and to a guard band (+-2^21 pixels around the viewport centre;
 * its fixed-point edge functions are defined up to +-2^22).  What remains undrawable is a vertex whose position is not finite. */
#define CRYCHIC_RASTER_COORD_OVERFLOW 1u   /* a post-clip vertex outside the +-2^22 pixel range (a non-finite position): triangle dropped */
#define CRYCHIC_RASTER_BAD_INDEX 2u        /* an index pointed outside the item's vertex buffer: triangle dropped */
int crychic_raster_status(crychic_ctx* ctx, void* stream, uint32_t* flags);

/* Ssao::ComputeSsao's blur iterations 1 .. blurCount - 1 run as ONE launch whose tiles wait for their neighbours' previous iteration
 * through per-tile counters in the edge workspace (Ssao.cpp:231-266 issues one draw per sweep and relies on the barrier between
 * draws).  The hand-off's contract ("Blur: one launch for the replayed iterations"): a tile's texels are stored
 * write-through, every wavefront waits for its stores (s_waitcnt vmcnt(0)) and reaches the workgroup barrier before one lane
 * publishes the counter; a waiting workgroup polls relaxed, then executes one agent-scope acquire, waits for it and passes a
 * barrier before any wavefront loads a neighbour's texel.  tools/handoff_isa.py checks that order in the emitted assembly.
 * The wait is bounded: a workgroup that gives up -- which would mean the device did not dispatch workgroups in grid order,
 * the assumption forward progress rests on -- records it and goes on.  This call synchronises `stream` and reports whether that
 * happened in the most recent chain issued on `ctx` (*timed_out = 1: that frame's ambient map is wrong).  Tests and bench.py
 * check it; CRYCHIC_BLUR_PER_ITERATION=1 in the environment selects one launch per iteration instead (the same pixels). */
int crychic_blur_chain_status(crychic_ctx* ctx, void* stream, uint32_t* timed_out);

/* All cascades of CRYCHIC::DrawSceneToShadowMap (CRYCHIC.cpp:2477-2510 loops over four) in one pass: passCBs[c].ViewProj and
 * shadow_dev[c] per cascade, the same items for all.  Bit-identical to nCascades calls of crychic_draw_scene_to_shadow_map;
 * the workspace must hold crychic_raster_workspace_bytes(nCascades * triangles, shadowDim, shadowDim).  nCascades is 1 .. 12
 * (gShadowMap[12], Common.hlsl:46: slots 4..11 hold the shadowed spot lights' maps); more than four targets run as consecutive
 * fused passes of at most four on `stream`. */
int crychic_draw_scene_to_shadow_maps(crychic_ctx* ctx, const crychic_pass_constants* passCBs, uint32_t nCascades,
                                      const crychic_draw_item* items, uint32_t nItems, uint32_t* const* shadow_dev, uint32_t shadowDim,
                                      int depthBias, float slopeScaledDepthBias, void* workspace_dev, size_t workspaceBytes, void* stream);

/* DrawNormalsAndDepth + DrawGBuffer in one rasterisation: the two passes draw the same items with the same ViewProj into
 * depth targets cleared to 1.0, so their visibility is identical; this entry rasterises once and runs both pixel shaders
 * on the winning primitive.  Every plane is bit-identical to calling the two passes one after the other. */
int crychic_draw_normals_depth_and_gbuffer(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                                           uint32_t nItems, const crychic_material_data* materials_dev, uint32_t nMaterials,
                                           const crychic_texture* textures, uint32_t nTextures, void* normal_dev, float* g0_dev,
                                           float* g1_dev, float* g2_dev, uint32_t* depth_dev, uint32_t W, uint32_t H,
                                           void* workspace_dev, size_t workspaceBytes, void* stream);

/* Strip-limited producers (SURVEY.md 8e "G-buffer for own strip only"; the reference scissors its passes to the whole client
 * area, CRYCHIC.cpp:2547-2548 -- with N GPUs each rank scissors the G-buffer pass to the rows it lights).  As the two entry
 * points above, but G0..G2 are produced for rows [gRow0, gRow0 + gRows) only; G-buffer texels outside those rows are left
 * untouched.  crychic_draw_gbuffer_rows also limits rasterisation and its depth target to the rows;
 * crychic_draw_normals_depth_and_gbuffer_rows still renders depth and view normals for the WHOLE frame (the SSAO taps of a
 * strip reach far outside it) and only skips the G-buffer stage elsewhere.  Inside the rows every plane is bit-identical to
 * the unscissored pass. */
int crychic_draw_gbuffer_rows(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                              uint32_t nItems, const crychic_material_data* materials_dev, uint32_t nMaterials,
                              const crychic_texture* textures, uint32_t nTextures, float* g0_dev, float* g1_dev, float* g2_dev,
                              uint32_t* depth_dev, uint32_t W, uint32_t H, uint32_t gRow0, uint32_t gRows, void* workspace_dev,
                              size_t workspaceBytes, void* stream);
int crychic_draw_normals_depth_and_gbuffer_rows(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                                                uint32_t nItems, const crychic_material_data* materials_dev, uint32_t nMaterials,
                                                const crychic_texture* textures, uint32_t nTextures, void* normal_dev, float* g0_dev,
                                                float* g1_dev, float* g2_dev, uint32_t* depth_dev, uint32_t W, uint32_t H,
                                                uint32_t gRow0, uint32_t gRows, void* workspace_dev, size_t workspaceBytes, void* stream);

/* The four G-buffer producers above with a format per plane: gbufferFlags = CRYCHIC_GBUFFER_G*_F16 bits (a set bit: that plane's
 * pointer addresses half4 texels, sized by crychic_gbuffer_plane_bytes); any other bit is CRYCHIC_E_INVALID_ARG.  normal_dev == NULL is
 * the G-buffer pass alone (crychic_draw_gbuffer_rows), otherwise the fused pass (crychic_draw_normals_depth_and_gbuffer_rows);
 * gRows == 0 is the whole target.  With gbufferFlags == 0 every plane is bit-identical to those entries; a half4 plane holds the
 * float4 plane's values rounded to nearest even (cleared texels: zero bits); depth, the normal map and float4 planes do not change. */
int crychic_draw_gbuffer_formats(crychic_ctx* ctx, const crychic_pass_constants* passCB, const crychic_draw_item* items,
                                 uint32_t nItems, const crychic_material_data* materials_dev, uint32_t nMaterials,
                                 const crychic_texture* textures, uint32_t nTextures, void* normal_dev, void* g0_dev, void* g1_dev,
                                 void* g2_dev, uint32_t gbufferFlags, uint32_t* depth_dev, uint32_t W, uint32_t H, uint32_t gRow0,
                                 uint32_t gRows, void* workspace_dev, size_t workspaceBytes, void* stream);

/* ---- environment capture (BUILD-DEFINED EXTENSION): the scene rendered into the cube map ------------- *
 * The reference's cube map is a file (CRYCHIC.cpp:960,968).  Here the library can produce it: six frames of the hot path, one per
 * face camera, written straight into level 0 of a chain whose further levels the device then builds.
 *
 * Mip chain.  The layout is crychic_load_dds_cube_rgba8_mips': level after level, each level the six faces (+X, -X, +Y, -Y, +Z, -Z)
 * of d_k = max(dim >> k, 1) squared RGBA8 texels.  Level k+1, face f, texel (x, y), channel c is (a + b + c' + d + 2) >> 2 over the
 * level-k texels (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1) of the same face, in integer arithmetic; when d_k is odd and
 * greater than 1 its last row and column are not read; the chain ends at a 1 x 1 level; nothing is filtered across faces. */
/* Bytes of the first `levels` levels of a dim-texel cube map's chain: the sum over k < levels of 6 * 4 * d_k^2.  Pure host
 * arithmetic (levels past the 1 x 1 level count 24 bytes each). */
size_t crychic_cube_chain_bytes(uint32_t dim, uint32_t levels);
/* Builds levels 1 .. levels - 1 of the chain at chain_dev from its level 0, in place, on `stream`: level 0 is read and never
 * written, no byte past level levels - 1 is touched, levels == 1 does nothing and succeeds.  ceil((levels - 1) / 6) launches.
 * levels is 1 .. min(15, floor(log2 dim) + 1); a NULL pointer, dim == 0, levels == 0 or more levels than the face size allows
 * return CRYCHIC_E_INVALID_ARG, dim > 32768 CRYCHIC_E_UNSUPPORTED.  chain_dev holds RGBA8 texels (4-byte aligned; 16-byte aligned
 * chains of faces whose size is a multiple of 4 take the 16-byte loads). */
int crychic_generate_cube_mips(crychic_ctx* ctx, uint8_t* chain_dev, uint32_t dim, uint32_t levels, void* stream);
/* The six face cameras of a capture at `pos` (host only): camera f has pos, aspect = 1, fovY = (float)(pi / 2), nearZ, farZ and
 *   face  +X        -X         +Y         -Y         +Z        -Z
 *   look  (1,0,0)   (-1,0,0)   (0,1,0)    (0,-1,0)   (0,0,1)   (0,0,-1)
 *   up    (0,1,0)   (0,1,0)    (0,0,-1)   (0,0,1)    (0,1,0)   (0,1,0)
 * -- the axes and ups of crychic_update_point_shadow_transforms, without its widening.  The constants of a face are what
 * crychic_update_main_pass_cb, crychic_update_ssao_cb and crychic_update_cascade_shadow_transform make of that camera at
 * W = H = dim.  Known answer: with depth all clear and CRYCHIC_LIGHT_SKY, the frame of camera f over a one-level cube map of the
 * frame's own dim is face f of that cube map, byte for byte (the sky pass of a face camera lands on texel centres).
 * Capture (Crychic.capture_environment, CRYCHIC::CaptureEnvironment): face f of level 0 of the destination is the RGBA8 frame
 * crychic_draw_hot_path* produces at dim x dim for camera f with CRYCHIC_LIGHT_SKY, out_rgba8_dev pointing at that face; planes and
 * cascades come from the producers with that camera; everything view-independent and the bound cube map (the source, which the
 * destination must not alias) are the main frame's; crychic_generate_cube_mips then builds the chain.
 * CRYCHIC_E_INVALID_ARG for a NULL pointer, a non-finite position, nearZ <= 0 or nearZ >= farZ. */
int crychic_cube_capture_cameras(const float pos[3], float nearZ, float farZ, crychic_camera cams[6]);

/* ---- cube map prefiltered by roughness (BUILD-DEFINED EXTENSION) --------------------------------------- *
 * Level k of a prefiltered chain holds the environment convolved with the GGX lobe of roughness rho = k / (levels - 1): the first
 * term of the split sum with N = V = R (Karis 2013), with the pass's own lobe (NDF_GGX is called with a = roughness: a^2 = rho^2).
 *
 * Sample table.  A pure function of (dim, levels, level k), 1 <= k < levels, computed on the host in double and stored as float.
 * For i = 0 .. 31: xi1 = (i + 0.5) / 32, xi2 = the base-2 radical inverse of i; cos^2(theta) = (1 - xi1) / (1 + (a^2 - 1) xi1),
 * phi = 2 pi xi2; the weight is w = 2 cos^2(theta) - 1 and a sample with w <= 0 is dropped.  A kept entry is { lx, ly, lz, lod }:
 * (lx, ly, lz) = (2 cos sin cos(phi), 2 cos sin sin(phi), w), the light direction in tangent space (lz is also the weight), and
 * lod = clamp(0.5 log2(Os / Op) + 1, 0, levels - 1) with Os = 1 / (32 D / 4), D = a^2 / (pi ((a^2 - 1) cos^2(theta) + 1)^2) and
 * Op = 4 pi / (6 dim^2).  *count is the number of kept entries (16 at the last level, whose weights sum to exactly 8), entries
 * past it are zero, and *rcpWeight = (float)(1 / sum of w), summed in double over the kept entries in index order.
 * CRYCHIC_E_INVALID_ARG for a NULL pointer, dim == 0, levels outside 2 .. 15 or level outside 1 .. levels - 1. */
int crychic_cube_prefilter_samples(uint32_t dim, uint32_t levels, uint32_t level, float samples[32][4], uint32_t* count,
                                   float* rcpWeight);   /* host only */
/* Prefiltered chain.  dst has the layout of src (crychic_cube_chain_bytes(dim, levels) bytes each); the two must not overlap.
 * Level 0 of dst is level 0 of src, byte for byte.  Texel (x, y) of face f of level k >= 1 (d = max(dim >> k, 1)):
 *   1. N = normalize of the direction of the texel centre: face coordinates (s, t) = ((2x + 1) / d - 1, (2y + 1) / d - 1) (the
 *      quotient is a * rcp(d)), major axis 1, the inverse of the cube sampler's face table: +X (1, -t, -s), -X (-1, -t, s),
 *      +Y (s, 1, t), -Y (s, -1, -t), +Z (s, -t, 1), -Z (-s, -t, -1);
 *   2. up = (0, 0, 1) if |N.z| < 0.999, else (1, 0, 0); T = normalize(up x N), B = N x T, every cross component one
 *      fma(a, b, -(c d));
 *   3. for the kept samples of level k's table in index order: L = lx T + ly B + lz N (per component a product and two mads, x
 *      then y then z), c = the trilinear chain lookup of src (all its levels) at direction L and level of detail lod_i, four
 *      channels, exactly as the lighting pass samples a chain; acc = fma(lz_i, c, acc) per channel;
 *   4. the texel is floor(saturate(acc * rcpWeight) * 255 + 0.5) per channel (one mad).
 * Texels are finite and the directions never degenerate (|N| = |L| = 1, lz > 0), so there is no NaN case.  src is meant to be a
 * box chain (crychic_generate_cube_mips or a DDS chain); any chain of the layout is accepted.  Nothing is filtered across faces.
 * One copy and levels - 1 launches on `stream`, nothing allocated: the call can be captured into a graph.  levels == 1 copies
 * level 0.  levels is 1 .. min(15, floor(log2 dim) + 1).  CRYCHIC_E_INVALID_ARG, before anything is enqueued, for a NULL pointer,
 * dim == 0, a chain that is not 4-byte aligned, levels out of range or overlapping chains; dim > 8192 (the lighting pass's limit
 * for a cube map it binds: the sampler's 32-bit offsets) CRYCHIC_E_UNSUPPORTED. */
int crychic_prefilter_cube_chain(crychic_ctx* ctx, const uint8_t* src_chain_dev, uint8_t* dst_chain_dev, uint32_t dim,
                                 uint32_t levels, void* stream);

/* ---- SH9 irradiance of a cube map (BUILD-DEFINED EXTENSION) --------------------------------------------- *
 * Monomials of a unit vector n = (x, y, z), in this order: b0 = 1, b1 = y, b2 = z, b3 = x, b4 = x y, b5 = y z,
 * b6 = fma(3 z, z, -1), b7 = x z, b8 = fma(x, x, -(y y)).  Constants K = { 1, 2, 2, 2, 15/4, 15/4, 5/16, 15/4, 15/16 } =
 * 4 pi c_m^2 A_l, c_m the real SH normalisation of monomial m and A = (1, 2/3, 1/4) the cosine lobe over pi; all exact in binary, so
 * a cube map of one colour c has ambient colour exactly c.
 *
 * Projection of one level (six faces of d x d RGBA8 texels, the chain's face order and layout).  For texel (x, y) of face f:
 *   dir = the direction of the texel centre (the prefilter's table above, step 1), r2 = dot(dir, dir) = fma(z, z, fma(y, y, x x)),
 *   n = dir * (1 / sqrt(r2)) (sqrt and reciprocal correctly rounded), w = 1 / (r2 * sqrt(r2)) -- the texel-centre solid angle up
 *   to the factor 4 / d^2, which cancels;
 *   q_m = the integer nearest to (w * b_m(n)) * 2^20 (one multiply, an exact scaling, ties to even), qw = the same of w * 2^20.
 * Sums, in 64-bit integers over all 6 d^2 texels: S_w = sum of qw;  S_{m,c} = sum of q_m * texel_c for c = r, g, b, texel_c the
 * byte 0 .. 255; alpha is ignored.  Integer sums are associative: the result depends on no lane, wave, workgroup or arrival order.
 * |S| < 2^58 at d = 8192.
 * Coefficient block: nine float4, 144 bytes, C_m = (r, g, b, 0),
 *   C_{m,c} = (float)((double)S_{m,c} * K_m / ((double)S_w * 255.0))
 * -- the conversions from int64 (exact below 2^53, correctly rounded above), one multiply, one multiply in the denominator, one
 * divide and the conversion to binary32 are all correctly rounded, on the device as on a host.
 *
 * Lookup (CRYCHIC_LIGHT_AMBIENT_SH): with n = the pixel's normalW, per channel e = C_0; e = fma(C_m, b_m(n), e) for m = 1 .. 8 in
 * index order; e = max(e, 0) (NaN -> 0: a zero-length normal has no ambient light);  amb_c = ambientAccess * e * albedo_c, the
 * product order of DeferredShading.hlsl:44.  The sky, the tone map, the reflection term, shininess and Fresnel are unchanged.
 *
 * Environment tail: CRYCHIC_CUBE_SH_BYTES bytes at crychic_cube_sh_offset(dim, levels) =
 * crychic_cube_chain_bytes(dim, max(levels, 1)) rounded up to 16, so a buffer of crychic_cube_chain_sh_bytes(dim, levels) = offset +
 * CRYCHIC_CUBE_SH_BYTES bytes holds a chain and its tail.  Bytes [0, 144) of the tail are the coefficient block; bytes [144, 368)
 * are the projection's 28 int64 accumulators (S_{m,c} at index 3 m + c, S_w at 27), scratch with no initialisation requirement;
 * bytes [368, 416) are the probe volume ("probe volume" below), which the projection leaves alone; the rest is reserved.  Both size
 * functions are pure host arithmetic. */
#define CRYCHIC_CUBE_SH_BYTES 512u
size_t crychic_cube_sh_offset(uint32_t dim, uint32_t levels);
size_t crychic_cube_chain_sh_bytes(uint32_t dim, uint32_t levels);
/* Projects the six d x d faces at level_dev -- any level of any chain: the caller adds crychic_cube_chain_bytes(dim, k) -- into the
 * tail at tail_dev.  Three short launches on `stream` (zero the accumulators, accumulate with one 64-bit integer atomic add per
 * quantity and workgroup, finalise), no allocation, no host read-back, no waiting between workgroups: capturable into a graph, and
 * projecting twice gives the same bits whatever the tail held.  1 <= d <= 8192.  CRYCHIC_E_INVALID_ARG, before anything is
 * enqueued, for a NULL pointer, d out of range, level_dev not 4-byte or tail_dev not 8-byte aligned, or a tail that overlaps the
 * level. */
int crychic_project_cube_sh(crychic_ctx* ctx, const uint8_t* level_dev, uint32_t d, void* tail_dev, void* stream);

/* ---- environment BRDF table (BUILD-DEFINED EXTENSION) ----------------------------------------------------- *
 * Level k of a prefiltered chain is the first factor of Karis' split sum; this table is the second: the integral of the pass's own
 * specular BRDF over the pass's own lobe, as a factor A of R0 and an offset B.  CRYCHIC_ENV_BRDF_BYTES = 4096 bytes: 32 x 32 dwords,
 * row-major; row j is roughness rho = (j + 0.5) / 32, column i is mu = N.V = (i + 0.5) / 32; each dword holds A | (B << 16), two R16
 * UNORM values.  It depends on nothing but this definition.  Lobe and masking are the pass's: NDF_GGX with a^2 = rho^2
 * (PBR.hlsl:4-14) and GeometrySmith with k = 0.125 (rho + 1) (rho + 1), that product order (PBR.hlsl:34).
 *
 * Quadrature: a product grid of 256 x 16 = 4096 samples per texel, xi_s = (s + 0.5) / 256 and phi_t = pi (t + 0.5) / 16 over the half
 * circle (V lies in the xz-plane, so only cos(phi) enters).  The sixteen cosines are these binary32 constants, no libm involved:
 * t = 0 .. 7: 0x3f7ec46d 0x3f74fa0b 0x3f61c598 0x3f45e403 0x3f226799 0x3ef15aea 0x3e94a031 0x3dc8bd36; t = 8 .. 15: the negations of
 * t = 7 .. 0.  Arithmetic is binary32 with fma, rcp (correctly rounded, flush-to-zero reciprocal) and len_from_sq (correctly rounded
 * square root of the argument clamped to [2^-100, 2^100]); nothing is fused unless written as fma.
 *   per texel:  a2m1 = fma(rho, rho, -1); omk = 1 - k; vz = mu; vx = len_from_sq(fma(-mu, mu, 1)); gV = rcp(fma(vz, omk, k));
 *   per s:      c2 = (1 - xi) * rcp(fma(a2m1, xi, 1)); c = len_from_sq(c2); sn = len_from_sq(1 - c2); rc = rcp(c);
 *   per (s, t): voh = fma(vx, sn * cos_t, vz * c); lz = fma(2 * voh, c, -vz); a sample with !(lz > 0) contributes nothing; otherwise
 *               gL = lz * rcp(fma(lz, omk, k)); gv = ((gV * gL) * voh) * rc; f = 1 - saturate(voh); fc = f f f f f, left to right;
 *               tB = fc * gv; tA = (1 - fc) * gv; qA, qB = the integers nearest to tA * 2^24 and tB * 2^24 (exact scaling, ties to
 *               even).
 * S_A = sum of qA and S_B = sum of qB are 64-bit integers; integer sums are associative, so no reduction order is part of the
 * definition.  A = float_to_unorm16((float)((double)S_A * 2^-36)), B alike: floor(saturate(x) * 65535 + 0.5) as one mad; both
 * conversions are exact or correctly rounded.  Every term is below 19.5, so q < 2^29 and |S| < 2^42; A lies in [0.0102, 0.9955], B in
 * [3.9e-8, 0.1441], and A + B <= 0.99548.  The quadrature's own error against a 2048 x 256 grid is at most 0.0024 in A (mean 0.0002;
 * worst at grazing angles near rho = 0.1) and 0.0002 in B, about half an RGBA8 step.
 *
 * Lookup (CRYCHIC_LIGHT_ENV_BRDF), per covered pixel: u = saturate(dot3(normalW, view)); v = saturate(roughness), the decoded value
 * the gloss lookup uses (NaN -> 0); (A, B) = the bilinear filter of the table at (u, v): t = fma(uv, 32, -0.5), floor and fraction,
 * indices clamped to [0, 31], each texel's halves decoded as R16 UNORM, lerp as one mad, x then y; spec_c = fma(R0_c, A, B);
 * lit_c = fma(spec_c, refl_c, tm_c) in place of DeferredShading.hlsl:97.  The sky, the tone map, the ambient term and the direct
 * lights are unchanged.
 *
 * The table travels with the cube map, behind the environment tail: crychic_cube_env_brdf_offset(dim, levels) =
 * crychic_cube_sh_offset(dim, levels) + CRYCHIC_CUBE_SH_BYTES, and a buffer of crychic_cube_chain_env_bytes(dim, levels) = that +
 * CRYCHIC_ENV_BRDF_BYTES bytes holds a chain, its tail and the table.  Both size functions are pure host arithmetic. */
#define CRYCHIC_ENV_BRDF_BYTES 4096u
size_t crychic_cube_env_brdf_offset(uint32_t dim, uint32_t levels);
size_t crychic_cube_chain_env_bytes(uint32_t dim, uint32_t levels);
/* Builds the table into the 4096 bytes at table_dev.  One launch on `stream`, no allocation, no context-owned buffer, no host
 * read-back: capturable into a graph, and building twice gives the same bits whatever the destination held.
 * CRYCHIC_E_INVALID_ARG, before anything is enqueued, for a NULL pointer or one that is not 4-byte aligned. */
int crychic_build_env_brdf(crychic_ctx* ctx, void* table_dev, void* stream);

/* ---- probe volume: box-projected reflections (BUILD-DEFINED EXTENSION) ---------------------------------- *
 * A capture taken at a position is looked up as if it were infinitely far away; box projection corrects that for one axis-aligned
 * proxy box around the capture.  A build definition: parity is against this repo's CPU checker (tests/parallax_ref).
 *
 * Probe volume: CRYCHIC_CUBE_PROBE_BYTES = 48 bytes of the environment tail's reserved area, at tail offset
 * CRYCHIC_CUBE_PROBE_OFFSET = 368: three float4, c = (cx, cy, cz, 0) the capture position, bmin = (.., 0) and bmax = (.., 0) the box.
 * Its address is cube_dev + crychic_cube_probe_offset(dim, levels) = cube_dev + crychic_cube_sh_offset(dim, levels) + 368 (pure host
 * arithmetic); a buffer of crychic_cube_chain_sh_bytes holds it, and so does one of crychic_cube_chain_env_bytes.  Tail bytes
 * [416, 512) stay reserved.  crychic_project_cube_sh writes tail bytes [0, 368) only.
 *
 * Correction (CRYCHIC_LIGHT_CUBE_PARALLAX), per covered pixel, in binary32 with rcp (above); nothing is fused unless written as fma.
 * p = posW, r = the reflection vector of DeferredShading.hlsl:94.
 *   for k = x, y, z: if |r_k| >= 2^-126 (false for NaN): e_k = (r_k < 0 ? bmin_k : bmax_k) - p_k, t_k = e_k * rcp(r_k); otherwise the
 *     component is skipped;
 *   t = +inf, then for k in order t = (t_k < t) ? t_k : t (a NaN t_k loses);  t = max(t, 0) (the clamp of HLSL's max);
 *   if !(t < +inf): r' = r -- nothing usable, the distant lookup;  otherwise h_k = fma(r_k, t, p_k), r'_k = h_k - c_k.
 * r' replaces r as the argument of the cube lookup alone (the trilinear fetch of the gloss chain).  The level from roughness,
 * f0 = 1 - saturate(dot(normalW, r)) and the whole reference weight, the split-sum (A, B) lookup, the ambient term, the sky, the
 * direct lights and the tone map stay on r, normalW, view and roughness as they are.  A zero or non-finite r' goes to the sampler
 * like any other direction.  There is no inside-the-box test, on purpose: rasterised floor positions sit an ulp either side of a box
 * face, and the clamp t >= 0 makes such a pixel reflect from its own position instead of flickering between two rules.
 * Known answers (exact), c = 0, bmin = (-4, -2, -4), bmax = (4, 6, 4): p = (1, -2, 1), r = (0.5, 0.5, 0) gives t = 6, r' = (4, 1, 1),
 * and so does r = (0.5, 0.5, -0.0f); r = (0, 0, 0) gives r' = r; p = (1, -2.5, 1), r = (0, -1, 0) clamps t to 0, r' = p - c. */
#define CRYCHIC_CUBE_PROBE_OFFSET 368u
#define CRYCHIC_CUBE_PROBE_BYTES 48u
size_t crychic_cube_probe_offset(uint32_t dim, uint32_t levels);
/* Writes the probe volume into the environment tail at tail_dev (cube_dev + crychic_cube_sh_offset(dim, levels)): bytes
 * [368, 416) of the tail and nothing else.  One tiny launch on `stream`: the twelve floats travel by value with the kernel's
 * arguments; no allocation, no host copy, capturable into a graph.  CRYCHIC_E_INVALID_ARG, before anything is enqueued, for a NULL
 * pointer, a tail_dev that is not 4-byte aligned, a non-finite value, or any component without boxMin < pos < boxMax strictly. */
int crychic_set_cube_probe_volume(crychic_ctx* ctx, void* tail_dev, const float pos[3], const float boxMin[3], const float boxMax[3],
                                  void* stream);

/* ---- procedural sky: a single-scattering atmosphere into the cube map (BUILD-DEFINED EXTENSION) ---------- *
 * The producer of level 0 of a cube map that needs neither a file nor six renders of a scene: one ray per texel through a spherical
 * atmosphere lit by one sun (Nishita-style single scattering: Rayleigh and Mie, no ozone, no multiple scattering), tone-mapped with
 * the lighting pass's own operator into RGBA8.  A build definition: nothing of it is the reference's, whose sky.hlsl only samples a
 * cube.  The device, a host build and the checker (tests/sky_ref) agree bit for bit.
 *
 * Float operations are IEEE binary32, each rounded once, in the order written; fma(a, b, c) is the fused a b + c and nothing else is
 * fused.  rcp, len_from_sq, dot3 and det_exp2 are those of crychic_fog below;  max0(x) = x > 0 ? x : 0 (NaN -> 0);
 * normalize3(v) = v * rcp(len_from_sq(dot3(v, v))) per component;  pow_inv_gamma is the lighting pass's pinned pow(x, 1 / 2.2)
 * (SCALE[E] * P(m - 1), gamma_pow.inc);  unorm8(x) = (uint32_t)fma(min(max(x, 0), 1), 255, 0.5).
 *
 * Atmosphere, in kilometres.  A planet of radius Rg = 6360 under a shell of radius Rt = 6420.  Rayleigh scattering
 * betaR = (5.8e-3f, 13.5e-3f, 33.1e-3f) per km with scale height 8; Mie scattering betaM = 21e-3f with extinction 1.1 betaM, scale
 * height 1.2 and g = 0.76.  The binary32 constants derived from them (nearest to the decimal written):
 *   Rg2 = 40449600 (exact);  invRg = 0.000157232702;  nHR = -0.180336878 (-log2(e) / 8);  nHM = -1.20224583 (-log2(e) / 1.2);
 *   tauR = (0.00836763065, 0.0194763839, 0.0477532074) (betaR log2(e));  tauM = 0.0333262533 (1.1 betaM log2(e));
 *   phaseR = 0.0596831031 (3 / (16 pi));  phaseM = 0.0195609424 (3 (1 - g^2) / (8 pi (2 + g^2)));  -2 g = -1.52;  1 + g^2 = 1.5776;
 *   invPi = 0.318309873.
 * Positions are carried as q = r^2 - Rg^2 (r the distance from the planet's centre), never as r, so that no height is the
 * difference of two numbers near 6400:   height(q) = q * rcp(len_from_sq(q + Rg2) + Rg).
 *
 * Host-side constants, once per call (double where written; every double operation is IEEE binary64, rounded once, in the order
 * written), with Nv = viewSteps, Ns = sunSteps, alt = altitude:
 *   len = sqrt(x x + y y + z z) of sunDir in double (left to right);  S = ((float)(x / len), (float)(y / len), (float)(z / len))
 *   r0 = 6360.0f + alt (binary32);  a0 = (float)(alt (12720.0 + alt));  cT = (float)((60.0 - alt) (12780.0 + alt));  r0Sy = r0 S.y
 *   invNv = 1.0f / (float)Nv;  invNv2 = invNv invNv;  invNs, invNs2 alike;  rd = rcp((float)dim)
 *   a2 = sunAngularRadius^2 in double;  cosDisc = (float)(1.0 - a2 (0.5 - a2 / 24.0));  groundK = (groundAlbedo invPi) sunIntensity
 * The observer stands at (0, r0, 0): +Y is up, as in the scene.
 *
 * Samples.  Both marches put sample i of N at the middle, in u, of the i-th of N equal intervals of u in [0, 1], with the distance
 * along the ray t = L u^2: denser near the start of the ray, where the air is densest for every ray that climbs.
 *   u_i = ((float)i + 0.5f) invN;   t_i = L (u_i u_i);   dt_i = L ((float)(2 i + 1) invN2)        (L the length of the ray's segment)
 *
 * blocked(q, bs) = bs < 0 && fma(bs, bs, -q) >= 0      -- the planet stands between the point (q, bs = P . S) and the sun
 * to_shell(c, b):  sq = len_from_sq(fma(b, b, c));  b >= 0 ? c rcp(sq + b) : sq - b      -- c = Rt^2 - r^2 >= 0, b = P . direction
 * sun_depth(q, bs, c), the sun march from a point:  L = to_shell(c, bs);  twob = bs + bs;  dR = dM = 0;  for j = 0 .. Ns - 1, with
 *   (s, ds) = sample j of Ns over L:  h = height(fma(s, s + twob, q));  dR = fma(det_exp2(h nHR), ds, dR);
 *   dM = fma(det_exp2(h nHM), ds, dM).
 * trans_c(dR, dM) = det_exp2(-fma(tauR_c, dR, tauM dM)), c = R, G, B.
 *
 * Texel (x, y) of face f of a dim-texel cube map:
 *   1  s = (float)(2 x + 1) rd - 1.0f;  t = (float)(2 y + 1) rd - 1.0f;  the direction of the texel centre is the prefilter's table
 *      (crychic_prefilter_cube_chain step 1): +X (1, -t, -s), -X (-1, -t, s), +Y (s, 1, t), -Y (s, -1, -t), +Z (s, -t, 1),
 *      -Z (-s, -t, -1);  v = normalize3 of it;  mu = dot3(v, S).
 *   2  b = r0 v.y;  twob = b + b;  dg = fma(b, b, -a0);  ground = b < 0 && dg >= 0;
 *      tEnd = ground ? a0 rcp(len_from_sq(dg) - b) : to_shell(cT, b).
 *   3  vR = vM = 0, sR_c = sM_c = 0.  For i = 0 .. Nv - 1, with (t, dt) = sample i of Nv over tEnd:
 *        w = t (t + twob);  q = a0 + w;  h = height(q);  rhoR = det_exp2(h nHR) dt;  rhoM = det_exp2(h nHM) dt;
 *        mR = fma(0.5f, rhoR, vR);  mM = fma(0.5f, rhoM, vM);  vR = vR + rhoR;  vM = vM + rhoM;
 *        bs = fma(t, mu, r0Sy);  a sample with blocked(q, bs) contributes nothing more (this is what makes twilight and night);
 *        otherwise  D = sun_depth(q, bs, max0(cT - w));  for each c:  T = trans_c(mR + D.dR, mM + D.dM);
 *        sR_c = fma(T, rhoR, sR_c);  sM_c = fma(T, rhoM, sM_c).
 *   4  m1 = fma(mu, mu, 1.0f);  phR = phaseR m1;  xg = fma(-1.52f, mu, 1.5776f);  phM = (phaseM m1) rcp(xg len_from_sq(xg))
 *      (Cornette-Shanks);  L_c = sunIntensity fma(phR betaR_c, sR_c, (phM betaM) sM_c).
 *   5  disc = !ground && mu >= cosDisc.  If ground or disc:  w = tEnd (tEnd + twob);  q = max0(a0 + w);  bs = fma(tEnd, mu, r0Sy);
 *      Tv_c = trans_c(vR, vM) (the whole view ray).  If ground && bs > 0 (the sun is above the ground point's horizon):
 *      D = sun_depth(q, bs, max0(cT - w));  L_c = L_c + ((groundK (bs invRg)) trans_c(D.dR, D.dM)) Tv_c.
 *      If disc:  L_c = fma(sunIntensity, Tv_c, L_c).
 *   6  e = L_c exposure;  byte_c = unorm8(pow_inv_gamma(e rcp(e + 1.0f)));  the texel is R | G << 8 | B << 16 | 255 << 24.
 * Every quantity is finite for parameters inside their ranges, so there is no NaN case.
 *
 * crychic_sky_sun_colour: zeros if blocked(a0, r0Sy); otherwise D = sun_depth(a0, r0Sy, cT) and rgb_c = sunIntensity trans_c(D.dR, D.dM).
 * Known answers: a sun 30 degrees below the horizon gives the sun colour (0, 0, 0) and every texel (0, 0, 0, 255); for a sun at the
 * zenith and altitude 0 the sun colour is sunIntensity exp(-(betaR_c 8 + 1.1 betaM 1.2)) up to the quadrature and the 60 km shell.
 *
 * Parameters: sunDir (towards the sun; any finite non-zero vector, normalised by the definition; default (0, 0.5, -0.8660254): 30
 * degrees up), altitude (0.002 km; 0 .. 50), sunIntensity (20; 0 .. 65536), exposure (2; 0 .. 65536), sunAngularRadius (0.02 rad;
 * 0 .. 0.5), groundAlbedo (0.3; 0 .. 1), viewSteps (16; 1 .. CRYCHIC_SKY_MAX_VIEW_STEPS), sunSteps (8; 1 .. CRYCHIC_SKY_MAX_SUN_STEPS),
 * reserved (must be 0).  crychic_sky_default_params fills the defaults (pure host code; CRYCHIC_E_INVALID_ARG for NULL). */
#define CRYCHIC_SKY_MAX_VIEW_STEPS 64
#define CRYCHIC_SKY_MAX_SUN_STEPS 32
typedef struct crychic_sky_params {
    float sunDir[3];
    float altitude;
    float sunIntensity;
    float exposure;
    float sunAngularRadius;
    float groundAlbedo;
    uint32_t viewSteps;
    uint32_t sunSteps;
    uint32_t reserved[2];
} crychic_sky_params;   /* 48 bytes */
int crychic_sky_default_params(crychic_sky_params* out);
/* Writes level 0 of faces [face0, face0 + faces) of the cube map at cube_dev (6 x dim x dim RGBA8, faces +X, -X, +Y, -Y, +Z, -Z; face
 * f starts at cube_dev + f dim dim 4) and no other byte; it reads no device memory.  A texel depends on nothing but (f, x, y, dim) and
 * the parameters, so any split of the six faces stitches to the whole call byte for byte; faces == 0 is valid and launches nothing.
 * params == NULL = the defaults.  One launch on `stream`: no allocation, no synchronisation, no host read-back; capturable into a
 * graph.  CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL cube_dev
 * or one that is not 4-byte aligned, dim outside 2 .. 8192, a face range outside the six faces, a parameter that is not finite or
 * outside its range, a zero sunDir, a non-zero reserved word. */
int crychic_render_sky(crychic_ctx* ctx, uint8_t* cube_dev, uint32_t dim, uint32_t face0, uint32_t faces,
                       const crychic_sky_params* params /* NULL = defaults */, void* stream);
/* The colour of the sun's light at the observer (above): the transmittance of the sun's own ray times sunIntensity, zeros when the
 * planet hides the sun.  Pure host code, the host build of the functions the kernel marches with: an integrator sets
 * Lights[0].Strength from it, so that the light reddens as the sky does.  params == NULL = the defaults.  CRYCHIC_E_INVALID_ARG for a
 * NULL rgb or a parameter crychic_render_sky refuses. */
int crychic_sky_sun_colour(const crychic_sky_params* params /* NULL = defaults */, float rgb[3]);

/* ---- post-process anti-aliasing of the back buffer (extension) ------------------------------------------
 * The reference's framework smooths edges with 4x MSAA (Common/d3dApp.cpp:190-191, :367, :518), which does not compose with a
 * deferred G-buffer; this is the deferred path's stand-in: one pass over the finished RGBA8 frame, a separate call after the
 * lighting pass.  FXAA-class, and defined entirely in 32-bit integer arithmetic, so the device, a host build and the checker
 * (tests/post_aa_ref) agree bit for bit.  A build definition: nothing of it is the reference's.
 *
 * in and out are RGBA8 planes, W x H, W and H >= 1 (odd sizes are valid: no half-resolution map is involved).  Every coordinate
 * clamps to the frame edge, never to the row range of a call.  Luma of a texel: L = 77 R + 150 G + 29 B (0 .. 65280).
 * For pixel (x, y), with M, N, S, E, W and NW, NE, SW, SE the lumas of its 3 x 3 neighbourhood:
 *   1 early copy    hi / lo = max / min of M, N, S, E, W; range = hi - lo.  If range == 0 or range < max(absMin, hi >> relShift):
 *                   out = in for this pixel (all four channels).
 *   2 orientation   horz = |NW - 2W + SW| + 2 |N - 2M + S| + |NE - 2E + SE|,  vert = |NW - 2N + NE| + 2 |W - 2M + E| + |SW - 2S + SE|;
 *                   the edge is horizontal iff horz >= vert.
 *   3 side          (a, b) = (N, S) if horizontal, else (W, E); gA = |a - M|, gB = |b - M|; the across-neighbour is the a side iff
 *                   gA >= gB; g = max(gA, gB); nb = the across-neighbour's luma; Lp = M + nb.
 *   4 end search    in each of the two directions along the edge, for i = 1 .. K: q = the pixel i steps along, q' = its neighbour on
 *                   the chosen side, d = L(q) + L(q') - Lp; stop at the first i with 2 |d| >= g.  The distance is that i, or K if no
 *                   step stopped; the end delta is the last d computed: (dn, en) for the negative direction, (dp, ep) for the positive.
 *   5 edge weight   (dmin, e) = (dn, en) if dn <= dp, else (dp, ep);  wE = 128 - (256 dmin) / (dn + dp) (integer division) if
 *                   (e < 0) != (M - nb < 0), else 0.
 *   6 sub-pixel     s = 2 (N + S + E + W) + NW + NE + SW + SE;  t = |s - 12 M|;  r = min(256, (256 t) / (12 range));
 *                   r2 = (r r (768 - 2 r)) >> 16;  wS = (((r2 r2) >> 8) subpix) >> 8.
 *   7 blend         w = max(wE, wS) (0 .. 256); per channel c: out_c = (in_c(x, y) (256 - w) + in_c(across-neighbour) w + 128) >> 8.
 * No intermediate exceeds 2^32.  Known answers: a uniform frame, or one whose ranges stay below the threshold, comes back unchanged;
 * a straight axis-aligned black / white edge changes only the two pixel columns (rows) beside it, each by w = 12 under the defaults.
 *
 * Parameters: absMin (default 2048, any value), relShift (3; 0 .. 31), searchSteps = K (12; 1 .. CRYCHIC_AA_MAX_SEARCH) and subpix
 * (192; 0 .. 256).  crychic_aa_default_params fills the defaults (pure host code; CRYCHIC_E_INVALID_ARG for NULL). */
#define CRYCHIC_AA_MAX_SEARCH 16
typedef struct crychic_aa_params { uint32_t absMin, relShift, searchSteps, subpix; } crychic_aa_params;   /* 16 bytes */
int crychic_aa_default_params(crychic_aa_params* out);
/* Writes output rows [row0, row0 + rows) of out_rgba8_dev and no other byte of it; in_rgba8_dev must hold valid pixels for rows
 * [row0 - 16, row0 + rows + 16) cut to [0, H), and no other row of it is read.  Stitched row ranges therefore equal the whole-frame
 * call byte for byte, for any row0 and rows.  params == NULL = the defaults.  One launch on `stream`: no allocation, no
 * synchronisation, no host read-back; capturable into a graph.  Planes are 4-byte aligned; with W a multiple of 4 and both planes
 * 16-byte aligned the pass moves 16 bytes per lane.  CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and
 * before anything is enqueued: a NULL pointer, a misaligned plane, W or H of 0, a row range outside the frame, a parameter outside
 * its range, in and out overlapping within W * H * 4 bytes.  More than 2^28 pixels or 2097120 rows: CRYCHIC_E_UNSUPPORTED. */
int crychic_antialias(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H,
                      uint32_t row0, uint32_t rows, const crychic_aa_params* params /* NULL = defaults */, void* stream);

/* ---- volumetric fog with sun shafts through the cascades (extension) ------------------------------------
 * One pass over the finished RGBA8 frame, a separate call after the lighting pass and before the anti-aliasing: every pixel is
 * attenuated by the fog between the eye and its surface (the far plane for sky), an ambient in-scatter term is added, and a sun
 * in-scatter term that counts only the samples of the view ray which the cascade maps say are lit.  Everything behind the lighting
 * pass is display-referred here (the tone map sits inside it), so the pass composes on RGBA8.  A build definition: nothing of it is
 * the reference's.  The device, a host build and the checker (tests/fog_ref) agree bit for bit.
 *
 * Float operations are IEEE binary32, each rounded once, in the order written; fma(a, b, c) is the fused a b + c and nothing else
 * is fused.  The named ones are the project's:
 *   rcp(b)          the correctly rounded 1 / b; |b| < 2^-126 gives +-inf, |b| > 2^126 gives +-0, NaN gives NaN
 *   len_from_sq(x)  the correctly rounded square root of x clamped to [2^-100, 2^100], NaN taken as 2^-100
 *   dot3(u, v)      fma(u.z, v.z, fma(u.y, v.y, u.x v.x))
 *   mulcol(x, y, z, w, m) = fma(w, m[3], fma(z, m[2], fma(y, m[1], x m[0])));   mulcol1(x, y, z, m) = fma(z, m[2], fma(y, m[1], x m[0])) + m[3]
 *   d24_to_float(u) with v = (float)(u & 0xFFFFFF): fma(v, C_hi, v C_lo), C_hi = 0x33800001 and C_lo = 0xA77FFFFF as bit patterns
 *                   (equal to the IEEE quotient v / 16777215 for every v)
 *   det_exp2(z)     for z not NaN: z clamped to [-125, 127], n = z rounded to the nearest integer (ties to even), f = z - n,
 *                   p = Horner in f with one fma per step over 0.00015406982856802642, 0.0013400138122960925, 0.009618260897696018,
 *                   0.05550328269600868, 0.24022649228572845, 0.6931471824645996, 1.0 (highest power first); the result is p 2^n
 * A matrix of the pass constants is stored transposed (column c of the row-vector matrix at floats 4c .. 4c + 3), as everywhere here.
 *
 * Host-side constants, once per call, with N = steps:  invN = 1.0f / (float)N;  c = -(density * 1.44269504f) * invN;
 * sx = 2.0f / (float)W;  sy = 2.0f / (float)H;  dimf = (float)shadowDim;  and for cascade j = 0 .. 3 and c in {x, y, z}:
 * a[j][c] = mulcol1(EyePosW, ShadowTransforms[j] + 4c).
 * Per pixel (px, py), Eye = EyePosW:
 *   1  d = d24_to_float(depth[py W + px])  (the top byte of the texel is ignored)
 *   2  nx = fma((float)px + 0.5f, sx, -1.0f);  ny = fma((float)py + 0.5f, -sy, 1.0f)
 *   3  h[c] = mulcol(nx, ny, d, 1.0f, InvViewProj + 4c), c = 0 .. 3;  rw = rcp(h[3]);  P = (h[0] rw, h[1] rw, h[2] rw).  A sky pixel
 *      (depth 1) is no special case: it reconstructs to the far plane.
 *   4  r = P - Eye;  L = len_from_sq(dot3(r, r)), in [2^-50, 2^50], never 0 or NaN;  Lc = fminf(L, maxDistance);  invL = rcp(L)
 *   5  q = det_exp2(c Lc);  qi = (uint32_t)fma(q, 65536.0f, 0.5f), in 0 .. 65536
 *   6  stepLen = Lc invN;  jit = ((float)B[py & 3][px & 3] + 0.5f) / 16.0f (exact), B the 4 x 4 Bayer matrix
 *      { 0, 8, 2, 10;  12, 4, 14, 6;  3, 11, 1, 9;  15, 7, 13, 5 }.  From here on everything but the sample coordinates is 32 / 64-bit
 *      integer arithmetic.
 *   7  T_0 = 65536, S = 0;  for i = 0 .. N - 1:  T_(i+1) = (T_i qi + 32768) >> 16 (the product in 64 bits);  w = T_i - T_(i+1) (>= 0);
 *      t = ((float)i + jit) stepLen;  S += lit(t) ? w : 0
 *   8  lit(t): the cascade is the lighting pass's own by distance from the eye: j = 0 if t < 30, 1 if t < 50, 2 if t < 80, 3 if
 *      t < 100, otherwise the sample is lit.  f = t invL;  for c in {x, y, z}, with m = ShadowTransforms[j] + 4c:
 *      b[c] = fma(r.z, m[2], fma(r.y, m[1], r.x m[0])),  s[c] = fma(b[c], f, a[j][c]);  fx = s.x dimf, fy = s.y dimf.  The sample is
 *      inside iff fx >= 0 && fx < dimf && fy >= 0 && fy < dimf (false for NaN).  A sample that is not inside is lit; one that is, is
 *      lit iff s.z <= d24_to_float(map[j][(uint32_t)fy shadowDim + (uint32_t)fx]).  One point compare: no filter, no bias (the
 *      samples are in open air), no blend between cascades.
 *   9  Tend = T_N;  for R, G, B:  o = (in Tend + ambient (65536 - Tend) + sun S + 32768) >> 16,  out = min(o, 255);  alpha is copied.
 * The sample's shadow coordinates are linear in f only because the cascade transforms are affine, so a ShadowTransforms[j], j < 4,
 * whose floats 12 .. 15 are not exactly (0, 0, 0, 1) is refused; crychic_update_cascade_shadow_transform followed by
 * crychic_update_main_pass_cb produces exactly that.
 * Known answers: density 0 gives qi = 65536 and out == in byte for byte.  N = 1, maxDistance = 0.5 (below the near plane's distance
 * of a camera with nearZ = 1), density such that c Lc == -1, maps full of 0xFFFFFF: q = 0.5, Tend = S = 32768 for every pixel,
 * out = min((in 32768 + (ambient + sun) 32768 + 32768) >> 16, 255); with maps full of 0, S = 0 and the sun term is gone.
 *
 * Parameters: density (default 0.02; finite, 0 .. 16), maxDistance (100; finite, > 0), steps = N (16; 1 .. CRYCHIC_FOG_MAX_STEPS),
 * ambient and sun (R, G, B in bytes 0 .. 2, byte 3 ignored; (70, 80, 100) and (150, 140, 110)), reserved (must be 0).
 * crychic_fog_default_params fills the defaults (pure host code; CRYCHIC_E_INVALID_ARG for NULL). */
#define CRYCHIC_FOG_MAX_STEPS 64
typedef struct crychic_fog_params {
    float density;
    float maxDistance;
    uint32_t steps;
    uint8_t ambient[4];
    uint8_t sun[4];
    uint32_t reserved[3];
} crychic_fog_params;   /* 32 bytes */
int crychic_fog_default_params(crychic_fog_params* out);
/* Writes rows [row0, row0 + rows) of out_rgba8_dev and no other byte; reads the same rows of in_rgba8_dev and depth_dev (W x H, D24 in
 * the low 24 bits), any texel of the four shadowDim x shadowDim maps, and InvViewProj, EyePosW and ShadowTransforms[0 .. 3] of cb (a
 * host pointer, read during the call).  Stitched row ranges therefore equal the whole-frame call byte for byte, for any row0 and
 * rows; rows == 0 launches nothing.  in == out (the same address) is valid: a pixel reads only its own texel.  params == NULL = the
 * defaults.  One launch on `stream`: no allocation, no synchronisation, no host read-back; capturable into a graph.
 * CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL plane, map or cb, a
 * plane or map that is not 4-byte aligned, W or H of 0, a row range outside the frame, shadowDim outside 1 ..
 * CRYCHIC_MAX_SPOT_SHADOW_DIM, a parameter outside its range or a non-zero reserved word, a cascade transform that is not affine, in and
 * out overlapping within W * H * 4 bytes other than in == out.  More than 2^28 pixels: CRYCHIC_E_UNSUPPORTED. */
int crychic_fog(crychic_ctx* ctx, const crychic_pass_constants* cb, const uint32_t* depth_dev, const uint32_t* const shadow_dev[4],
                uint32_t shadowDim, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0,
                uint32_t rows, const crychic_fog_params* params /* NULL = defaults */, void* stream);

/* ---- screen-space reflections of the lit frame (extension) -------------------------------------------------
 * One pass over the finished RGBA8 frame, a separate call after the lighting pass and before the fog: a pixel whose surface is
 * smooth enough follows its mirrored view ray across the depth plane and, where the ray meets a surface on screen, blends the
 * frame's texel there over its own, weighed by the surface's Fresnel term and faded towards the border of the frame and the end of
 * the ray.  The lighting pass adds its reflection term after the tone map, so the blend is display-referred like that term.  A build
 * definition: nothing of it is the reference's.  The device, a host build and the checker (tests/ssr_ref) agree bit for bit.
 *
 * Float operations are IEEE binary32, each rounded once, in the order written; fma is fused only where written.  rcp, len_from_sq,
 * dot3, mulcol and d24_to_float are those of crychic_fog; lerpf, saturate, clampf and normalize3 those of crychic_apply_decals;
 * reflect3(i, n) = (fma(-t, n.x, i.x), fma(-t, n.y, i.y), fma(-t, n.z, i.z)) with t = 2.0f dot3(n, i).  x / w below stands for x rcp(w).
 *
 * Host side, once per call, with N = steps:  A = cb->Proj[10], B = cb->Proj[11] in memory order (viewZ = B / (d - A), as in
 * crychic_dof), both finite and B != 0;  sx = 2.0f / (float)W;  sy = 2.0f / (float)H;  Wf = (float)W;  Hf = (float)H;  hw = Wf 0.5f;
 * hh = Hf 0.5f;  invN = 1.0f / (float)N;  wmin = cb->NearZ.
 * Per pixel (px, py), Eye = EyePosW, with in, depth and the G-buffer planes indexed by py W + px:
 *   1  u = depth & 0xFFFFFF;  rough = G1.w.  If u == 0xFFFFFF (sky) or !(rough < maxRoughness) (so for a NaN too):  out = in.
 *   2  d = d24_to_float(u);  P = the world point of crychic_fog's steps 2 and 3;  V = normalize3(P - Eye);  Nw = normalize3(G2.xyz);
 *      R = reflect3(V, Nw);  Q.c = fma(R.c, maxDistance, P.c).
 *   3  h0[c] = mulcol(P.x, P.y, P.z, 1.0f, ViewProj + 4c), c = 0 .. 3, and h1 likewise of Q.  If h1.w < wmin:
 *      tt = (h0.w - wmin) rcp(h0.w - h1.w);  md = maxDistance tt;  Q.c = fma(R.c, md, P.c);  h1 again of that Q (once: no second test).
 *      If !(h0.w > wmin):  out = in.  screen(h) = (fma(h.x / h.w, hw, hw), fma(-(h.y / h.w), hh, hh), h.z / h.w): pixels and NDC
 *      depth, which is affine along a line of the screen.  s0 = screen(h0);  ds = screen(h1) - s0.  The sample at t is
 *      x = fma(ds.x, t, s0.x), y = fma(ds.y, t, s0.y), dr = fma(ds.z, t, s0.z);  it is ok iff
 *      x >= 0 && x < Wf && y >= 0 && y < Hf && dr < 1.0f (false for a NaN), and then its pixel is ((uint32_t)x, (uint32_t)y).
 *   4  jit as in crychic_fog's step 6 (the same Bayer matrix).  For i = 0 .. N - 1:  t_i = ((float)i + jit) invN.  A sample that is
 *      not ok ends the ray: no hit.  A sample in (px, py) itself is skipped.
 *   5  Otherwise, with v the low 24 bits of the sample pixel's depth word and dz = d24_to_float(v):  D = (dr - A) (dz - A);
 *      n = B (dz - dr);  the sample is a hit iff  v != 0xFFFFFF && dr > dz && bias D <= n && n <= thickness D  -- the test
 *      bias <= viewZ(dr) - viewZ(dz) <= thickness without a reciprocal per step.  The first hit, at i = I, ends the march.
 *   6  lo = (I == 0) ? 0.0f : t_(I-1);  hi = t_I;  the hit pixel is t_I's.  CRYCHIC_SSR_REFINE times:  tm = (lo + hi) 0.5f;  if the
 *      sample at tm is ok, not in (px, py) and passes the test of step 5 on its own pixel:  hi = tm and the hit pixel is tm's;
 *      else lo = tm.  t_hit = hi;  (hx, hy) the hit pixel;  hit = in[hy W + hx], a point sample.
 *   7  per channel c of albedo = G1.xyz, with metalness = G0.w:  R0 = lerpf(0.04f, albedo_c, metalness);
 *      f0 = 1.0f - saturate(dot3(Nw, R));  f2 = f0 f0;  f5 = (f2 f2) f0;  w = (1.0f - rough) fma(1.0f - R0, f5, R0);
 *      wq = (uint32_t)fma(clampf(w, 0.0f, 1.0f), 65536.0f, 0.5f), 0 .. 65536.  From here on unsigned integers.
 *   8  e = min(hx, W - 1 - hx, hy, H - 1 - hy);  fe = min(e, E) 65536 / E with E = edgeFade (floor);  tq = (uint32_t)(t_hit 65536.0f);
 *      fd = min(65536, 4 (65536 - tq));  K = ((((wq fe) >> 16) fd) >> 16) intensity >> 8, the two inner products in 64 bits; 0 .. 65536.
 *   9  out = (in (65536 - K) + hit K + 32768) >> 16 for R, G, B;  alpha is the pixel's own.  No hit:  out = in.
 * Known answers: maxRoughness 0, a depth plane of sky or intensity 0 give out == in byte for byte; a frame of one colour stays
 * that colour under any G-buffer, depth and parameters; alpha is always the pixel's own.
 * Known limits: the pass reflects only what is on screen and in front; a thin object can fall between two samples; a hit is
 * weighed by the surface's own Fresnel term and blended OVER the frame, so the cube-map reflection the lighting pass added stays
 * under the blend and is not removed; the hit colour is not blurred by roughness.
 *
 * Parameters: maxDistance (world units, default 20; finite, > 0), thickness (view units, 0.5; finite, > 0), bias (0.02; >= 0 and
 * below thickness), maxRoughness (0.75; 0 .. 1), steps = N (32; 1 .. CRYCHIC_SSR_MAX_STEPS), edgeFade = E (pixels, 32; 1 .. 1024),
 * intensity (256; 0 .. 256), reserved (must be 0).  crychic_ssr_default_params fills the defaults (pure host code;
 * CRYCHIC_E_INVALID_ARG for NULL). */
#define CRYCHIC_SSR_MAX_STEPS 64
#define CRYCHIC_SSR_REFINE 4
typedef struct crychic_ssr_params {
    float maxDistance;
    float thickness;
    float bias;
    float maxRoughness;
    uint32_t steps;
    uint32_t edgeFade;
    uint32_t intensity;
    uint32_t reserved;
} crychic_ssr_params;   /* 32 bytes */
int crychic_ssr_default_params(crychic_ssr_params* out);
/* Writes rows [row0, row0 + rows) of out_rgba8_dev and no other byte; reads ANY row of in_rgba8_dev and depth_dev (W x H, D24 in the
 * low 24 bits) -- the frame, not the row range --, the same rows of the three G-buffer planes, and Proj, ViewProj, InvViewProj, EyePosW
 * and NearZ of cb (a host pointer, read during the call).  Stitched row ranges therefore equal the whole-frame call byte for byte, for
 * any row0 and rows; rows == 0 launches nothing.  flags carries only CRYCHIC_GBUFFER_G*_F16 bits: a set bit says that plane's pointer
 * addresses half4 texels, which widen exactly on read as in the lighting pass, so every format mix equals the call on the widened
 * planes bit for bit.  in and out must not overlap at all within W * H * 4 bytes: a pixel reads other pixels' texels.  params == NULL
 * = the defaults.  One launch on `stream`: no allocation, no synchronisation, no host read-back; capturable into a graph.
 * CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL plane or cb, a
 * G-buffer plane that is not 16-byte (half4: 8-byte) aligned, a depth or frame plane that is not 4-byte aligned, W or H of 0, a row
 * range outside the frame, a parameter outside its range or a non-zero reserved word, unknown flag bits, in and out overlapping, a
 * non-finite Proj[10] or Proj[11] or Proj[11] == 0.  More than 2^28 pixels, or more than 2^22 columns or rows: CRYCHIC_E_UNSUPPORTED. */
int crychic_ssr(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev, const float* g2_dev,
                const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0,
                uint32_t rows, uint32_t flags, const crychic_ssr_params* params /* NULL = defaults */, void* stream);

/* ---- glossy screen-space reflections: a blurred pyramid of the lit frame and a cone lookup (extension) ------
 * crychic_ssr takes the hit colour as a point sample whatever the surface's roughness.  crychic_ssr_pyramid builds a binomial
 * pyramid of the finished RGBA8 frame; crychic_ssr_glossy is crychic_ssr with the hit colour fetched from the level whose texel is as
 * wide as the reflection cone at the hit.  A build definition: nothing of it is the reference's.  The device, a host build and the
 * checker (tests/ssr_gloss_ref) agree bit for bit.
 *
 * The pyramid, all unsigned 32-bit integers.  Level 0 is the frame itself and is never copied.  W_k = (W_(k-1) + 1) >> 1, H_k
 * likewise (the bloom's sizes).  `levels` counts level 0: 1 .. CRYCHIC_SSR_GLOSS_MAX_LEVELS.  n_eff, the highest level built, is the
 * smaller of levels - 1 and the first k with W_k == H_k == 1 (0 for a 1 x 1 frame): levels = 1 builds nothing.  A texel is RGBA8 and
 * all four channels are filtered alike.  Level k + 1 from level k is the bloom's 4 x 4 binomial (1, 3, 3, 1) x (1, 3, 3, 1):
 * destination (x, y) reads source columns 2x - 1 .. 2x + 2 and rows 2y - 1 .. 2y + 2, each coordinate clamped to the source level's
 * edge;  sum = the 16 products (at most 64 * 255);  v = (sum + 32) >> 6 per channel.
 * Workspace: levels 1 .. n_eff back to back, each starting on a 16-byte boundary; level k is W_k x H_k texels of 4 bytes, row-major.
 * crychic_ssr_pyramid_bytes is the end of level n_eff (0 when n_eff is 0), crychic_ssr_pyramid_offset the start of level k (0 for
 * k = 0 or k > n_eff, as for W or H of 0 or levels outside 1 .. CRYCHIC_SSR_GLOSS_MAX_LEVELS); both are pure host code.
 * Known answers: a frame of one colour has that colour in every texel of every level; transposing the frame transposes every
 * level; a frame whose columns alternate 0 and 255 has 128 in every level-1 texel whose four source columns are unclamped
 * ((4 * 8 * 255 + 32) >> 6); on a frame affine in x and y a level-k texel whose level-0 support (4 * 2^k - 3 columns and rows about
 * its centre) lies inside the frame is within k / 2 of the affine value at its centre.
 *
 * The glossy pass.  Steps 1 to 6 of crychic_ssr stand: the same ray, the same hit pixel (hx, hy), the same t_hit.  Steps 7 to 9
 * stand too.  Between them only the source of `hit` changes; rough is step 1's, len_from_sq crychic_fog's, det_log2
 * crychic_apply_decals':
 *   6a  dx = (float)hx - (float)px;  dy = (float)hy - (float)py;  Lpx = len_from_sq(fma(dx, dx, dy dy));
 *       r = (coneScale rough) Lpx  -- the lighting pass's lobe is NDF_GGX with a = roughness, not squared (section 15), so the cone's
 *       tangent goes with rough; the cone's length is taken as the ray's length on the screen;
 *       lam = r > 1.0f ? det_log2(r) : 0.0f (a NaN gives 0);  lam = lam < (float)n_eff ? lam : (float)n_eff;
 *       lq = (uint32_t)fma(lam, 256.0f, 0.5f);  k = lq >> 8;  f = lq & 255 (0 when k == n_eff, since lq <= 256 n_eff).
 *   6b  integers only.  fetch(k), along x:  T = ((2 hx + 1) 128) >> k;  U = max(T, 128) - 128  -- (hx + 1/2) / 2^k - 1/2 in 1/256
 *       texel, clamped at 0;  x0 = min(U >> 8, W_k - 1);  x1 = min(x0 + 1, W_k - 1);  fx = U & 255;  y0, y1, fy likewise from hy and
 *       H_k.  Per channel, with cXY the level's texel (xX, yY):  top = c00 (256 - fx) + c10 fx;  bot = c01 (256 - fx) + c11 fx;
 *       v_k = (top (256 - fy) + bot fy + 32768) >> 16.  At k = 0 this is in[hy W + hx] exactly.
 *       hit_c = f == 0 ? v_k : (v_k (256 - f) + v_(k+1) f + 128) >> 8.
 * The pyramid is always that of the whole frame `in`, built with the same W, H and levels.
 * Known answers: coneScale 0, levels 1, or a G1 plane with roughness 0 everywhere each give crychic_ssr's output byte for byte on
 * any input; a frame of one colour stays that colour; alpha is always the pixel's own.
 * Known limit: the pyramid blurs across depth edges, so a rough floor's reflection of a box can pick up some floor colour.
 *
 * Parameters: coneScale (finite, 0 .. 16; default 0, the sharp pass: the measurement that was to set it, tests/ssr_gloss_quality.py,
 * leaves no pixel to measure at any roughness of its grid (profiles/ssr_gloss_quality.txt), so the pass is EXPERIMENTAL and the
 * caller chooses the cone), levels (6; 1 .. CRYCHIC_SSR_GLOSS_MAX_LEVELS), reserved (must be 0).  crychic_ssr_gloss_default_params fills the defaults (pure host code;
 * CRYCHIC_E_INVALID_ARG for NULL). */
#define CRYCHIC_SSR_GLOSS_MAX_LEVELS 8
typedef struct crychic_ssr_gloss_params {
    float coneScale;
    uint32_t levels;
    uint32_t reserved[2];
} crychic_ssr_gloss_params;   /* 16 bytes */
int crychic_ssr_gloss_default_params(crychic_ssr_gloss_params* out);
size_t crychic_ssr_pyramid_bytes(uint32_t W, uint32_t H, uint32_t levels);
size_t crychic_ssr_pyramid_offset(uint32_t W, uint32_t H, uint32_t levels, uint32_t k);
/* crychic_ssr_pyramid: after it level k of workspace_dev holds level k of in_rgba8_dev's pyramid for k = 1 .. n_eff; no other byte
 * of the workspace is written (not the gaps between levels either) and in_rgba8_dev is only read.  n_eff launches on `stream`, one
 * behind the other; no allocation, no synchronisation, no host read-back; capturable into a graph.  workspace_dev may be NULL only
 * where crychic_ssr_pyramid_bytes(W, H, levels) is 0 (nothing is launched then).
 * CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL plane or (where
 * bytes are needed) workspace; a plane that is not 4-byte aligned or a workspace that is not 16-byte aligned; W or H of 0; levels
 * outside its range; workspace_bytes below crychic_ssr_pyramid_bytes(W, H, levels); a workspace (its first
 * crychic_ssr_pyramid_bytes bytes) overlapping the plane.  More than 2^28 pixels: CRYCHIC_E_UNSUPPORTED. */
int crychic_ssr_pyramid(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint32_t W, uint32_t H, uint32_t levels, void* workspace_dev,
                        size_t workspace_bytes, void* stream);
/* crychic_ssr_glossy: crychic_ssr's contract in every word -- the planes it reads and writes, the row range (stitched ranges equal
 * the whole frame; the pyramid is always of the whole frame), flags, params, its refusals -- with two more arguments: pyramid_dev,
 * what crychic_ssr_pyramid(in_rgba8_dev, W, H, gloss->levels) left (only read; any texel of it), and gloss (NULL = the defaults).
 * Refused besides, with CRYCHIC_E_INVALID_ARG: a coneScale that is not finite or outside 0 .. 16, levels outside its range, a
 * non-zero reserved word, a NULL pyramid where bytes are needed, a pyramid that is not 16-byte aligned, pyramid_bytes below
 * crychic_ssr_pyramid_bytes(W, H, levels), a pyramid overlapping out_rgba8_dev.  One launch. */
int crychic_ssr_glossy(crychic_ctx* ctx, const crychic_pass_constants* cb, const float* g0_dev, const float* g1_dev,
                       const float* g2_dev, const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, const void* pyramid_dev,
                       size_t pyramid_bytes, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                       uint32_t flags, const crychic_ssr_params* params /* NULL = defaults */,
                       const crychic_ssr_gloss_params* gloss /* NULL = defaults */, void* stream);

/* ---- depth of field from the depth plane (extension) -------------------------------------------------------
 * One pass over the finished RGBA8 frame, a separate call after the lighting pass (and the fog) and before the anti-aliasing: a
 * thin-lens blur.  Every texel has a circle of confusion from its depth; every output pixel gathers the texels of a disc of radius R
 * around it, each weighed by how far its own circle reaches, with the rule that a sample behind the pixel cannot spread over it
 * further than the pixel itself is blurred (a sharp foreground stays sharp in front of a blurred background) while a sample in front
 * spreads with its own circle (a blurred foreground bleeds over what is behind it).  A build definition: nothing of it is the
 * reference's.  The device, a host build and the checker (tests/dof_ref) agree bit for bit.
 *
 * Float operations are IEEE binary32, each rounded once, in the order written; nothing is fused except inside d24_to_float (see
 * crychic_fog above: fma(v, C_hi, v C_lo) with v = (float)(u & 0xFFFFFF), the IEEE quotient v / 16777215; the top byte is ignored).
 * clampf(x, lo, hi) = fminf(fmaxf(x, lo), hi), so a NaN gives lo.
 *
 * Host side, once per call:  A = cb->Proj[10], B = cb->Proj[11] in memory order (the two numbers of the SSAO pass's ndc_to_view:
 * viewZ = B / (d - A)), both finite and B != 0;  g = focusDistance / B (IEEE division);  ap16 = aperture * 16.0f;
 * hi = (float)(16 R) with R = maxRadius.
 * Circle of confusion of a depth texel, c = 0 .. 16 R <= 128, in 1/16 pixel:
 *   d = d24_to_float(depth);  x = (d - A) g  (= focusDistance / viewZ, the thin-lens term, without a reciprocal per texel);
 *   e = fabsf(1.0f - x);  u = e ap16;  c = (uint32_t)(clampf(u, 0.0f, hi) + 0.5f).
 * Tables, pure integer:  for every offset o = (ox, oy) with ox^2 + oy^2 <= R^2 (5, 13, 29, 49, 81, 113, 149, 197 offsets at
 * R = 1 .. 8):  d16(o) = isqrt(256 (ox^2 + oy^2)), the floor integer square root;  inv[c] = 2^20 / max(c, 16)^2 (floor) for
 * c = 0 .. 128, so inv[0 .. 16] = 4096, inv[17] = 3628, inv[64] = 256, inv[128] = 64.
 * Per output pixel p, with D_p the low 24 bits of its depth word and c_p its circle of confusion: over every offset o of the disc
 * whose sample s = p + o lies inside the FRAME [0, W) x [0, H) -- the frame, not the row range of the call; a sample outside it is
 * skipped:
 *   c_e = (D_s > D_p) ? min(c_s, c_p) : c_s;   k = clamp((int)c_e + 8 - (int)d16(o), 0, 16);   w = k inv[c_e];
 *   Sw += w;   S_ch += w in_s[ch]  for R, G, B.
 * The sums are 32-bit unsigned.  The centre tap has c_e = c_p, d16 = 0 and k = min(c_p + 8, 16) >= 8, so Sw >= min over c of
 * min(c + 8, 16) inv[c] = 16 inv[128] = 1024 > 0;  w <= 16 * 4096, so the largest channel sum is 197 * 16 * 4096 * 255 =
 * 3 292 200 960 < 2^32, and adding Sw >> 1 (at most 197 * 32768) does not reach 2^32 either.
 *   out[ch] = (S_ch + (Sw >> 1)) / Sw  for R, G, B;   alpha is the pixel's own input alpha.
 * Integer sums make the result independent of the order of the taps, which is what lets the kernel reorder and skip them.
 * Known answers: aperture 0 gives out == in byte for byte (a tap other than the centre has d16 >= 16 and needs c_e >= 9 to weigh
 * anything); a frame of one colour stays that colour under any depth and parameters; a depth step with the near half at c = 0 and
 * the far half at c = 128 gives the near half back byte for byte and changes the far half; with the near half at c = 128 and the far
 * half at c = 0 the far pixels more than 8 columns from the step come back byte for byte and those within 8 columns change; under
 * constant depth an input symmetric under the eight symmetries of the square lattice gives a symmetric output.
 *
 * Parameters: focusDistance (view-space units, default 15; finite, > 0), aperture (the circle-of-confusion radius in pixels of a
 * point at infinity, default 6; finite, 0 .. 64), maxRadius = R (pixels, default 8; 1 .. CRYCHIC_DOF_MAX_RADIUS), reserved (must be
 * 0).  crychic_dof_default_params fills the defaults (pure host code; CRYCHIC_E_INVALID_ARG for NULL). */
#define CRYCHIC_DOF_MAX_RADIUS 8
typedef struct crychic_dof_params {
    float focusDistance;
    float aperture;
    uint32_t maxRadius;
    uint32_t reserved[5];
} crychic_dof_params;   /* 32 bytes */
int crychic_dof_default_params(crychic_dof_params* out);
/* Writes rows [row0, row0 + rows) of out_rgba8_dev and no other byte; reads rows [row0 - R, row0 + rows + R) cut to [0, H) of
 * in_rgba8_dev and depth_dev (W x H, D24 in the low 24 bits), and Proj of cb (a host pointer, read during the call).  Stitched row
 * ranges equal the whole-frame call byte for byte, for any row0 and rows; rows == 0 launches nothing.  in and out must not overlap
 * at all within W * H * 4 bytes: a pixel reads its neighbours.  params == NULL = the defaults.  One launch on `stream`: no
 * allocation, no synchronisation, no host read-back; capturable into a graph.
 * CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL plane or cb, a
 * plane that is not 4-byte aligned, W or H of 0, a row range outside the frame, a parameter outside its range or a non-zero reserved
 * word, a non-finite Proj[10] or Proj[11] or Proj[11] == 0, in and out overlapping.  More than 2^28 pixels: CRYCHIC_E_UNSUPPORTED. */
int crychic_dof(crychic_ctx* ctx, const crychic_pass_constants* cb, const uint32_t* depth_dev, const uint8_t* in_rgba8_dev,
                uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                const crychic_dof_params* params /* NULL = defaults */, void* stream);

/* ---- deferred decals (extension) ---------------------------------------------------------------------------
 * One pass over the G-buffer planes, a separate call between the producer passes and the lighting pass: oriented boxes project
 * RGBA8 textures onto whatever surface lies inside them and blend albedo, roughness, metalness and the normal of the planes in
 * place.  A build definition: nothing of it is the reference's.  The device, a host build and the checker (tests/decal_ref) agree
 * bit for bit.  The SSAO pass's own view-normal map is NOT touched: ambient occlusion sees the surface without the decals' normals.
 *
 * Float operations are IEEE binary32, each rounded once, in the order written; fma is fused only where written.  Primitives:
 *   mulcol1 as under crychic_fog;  dot3(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x b.x));  lerpf(a, b, t) = fma(t, b - a, a);
 *   saturate(x) = 0 for x <= 0 or NaN, 1 for x >= 1, else x;  clampf(x, lo, hi) = fminf(fmaxf(x, lo), hi), so a NaN gives lo;
 *   clampi the same on integers;
 *   normalize3(v) = v.c * inv for each c with inv = 1 / sqrtf(L), L = dot3(v, v) clamped to [2^-100, 2^100] (a NaN gives 2^-100),
 *   square root and quotient correctly rounded: the zero vector stays zero;
 *   unorm8_to_float(b) = (float)b / 255 (IEEE);  half_to_float exact;  float_to_half round to nearest even;
 *   det_log2(x): -inf for +-0 and positive subnormals, NaN for negative x and NaN, else with bits(x) - 0x3F3504F3 = ue:
 *     ef = (float)((int32_t)ue >> 23), m = float of bits (ue & 0x7FFFFF) + 0x3F3504F3, s = (m - 1) * (1 / (m + 1)), s2 = s s,
 *     p = fma(fma(fma(0.43174004554748535f, s2, 0.5767142176628113f), s2, 0.9617988467216492f), s2, 2.885390043258667f),
 *     result fma(s, p, ef);
 *   bilinear_setup(u, v, w, h) for finite u, v: tx = fma(u, (float)w, -0.5f), i0 = (int)floorf(tx), fx = tx - floorf(tx); ty, j0, fy
 *     likewise with v and h;  bilerp(t00, t10, t01, t11, fx, fy) = lerpf(lerpf(t00, t10, fx), lerpf(t01, t11, fx), fy).
 *
 * A decal is an oriented box: the image of the unit cube [-1/2, 1/2]^3 under an affine map.  It looks down its local -z and lands
 * on surfaces whose normals point towards normalW; the texture's u runs along local +x, v against local +y.  The array is DEVICE
 * memory the caller uploads (as the local lights are), at most CRYCHIC_MAX_DECALS entries.
 *
 * Host side, once per call:  pix = 2.0f / (Proj[5] * (float)H) with H the frame height;  Vz = View + 8 (four floats).
 * Per pixel of the call's rows:
 *  0. Covered iff (depth & 0xFFFFFF) < 0xFFFFFF; otherwise nothing further is read and nothing is written.  G0, G1, G2 are loaded in
 *     their formats (half texels widened exactly).  P = G0.xyz;  n0 = normalize3(G2.xyz);  running values alb = G1.xyz,
 *     rough = G1.w, metal = G0.w, nrm = n0;  s = mulcol1(P.x, P.y, P.z, Vz) * pix  (the world-space size of a pixel at P's view depth).
 * Then for d = 0 .. nDecals - 1 in ASCENDING order (a later decal lies over an earlier one):
 *  1. texture >= nTextures: the decal changes nothing.
 *  2. Bounds: P.c >= boundsMin[c] && P.c <= boundsMax[c] for c = 0 .. 2 (false for a NaN on either side); otherwise the decal changes
 *     nothing.  The bounds are part of the definition, not a hint: a caller that sets them narrower than the box cuts the decal.
 *  3. q[c] = mulcol1(P.x, P.y, P.z, invWorld + 4c), c = 0 .. 2.  Inside iff fabsf(q[c]) <= 0.5f for all c; otherwise nothing.
 *  4. fade = saturate(fma(dot3(n0, normalW), fadeScale, fadeBias)).  Always n0, never the running normal.
 *  5. u = q[0] + 0.5f;  v = 0.5f - q[1].
 *  6. t = sample(textures[texture]), where sample(T) with L = max(mipLevels, 1) levels in the layout of crychic_texture is
 *       L == 1: fetch(0);  otherwise  lod = clampf(det_log2(s * texelsPerUnit), 0.0f, (float)(L - 1))  (NaN and -inf give 0),
 *       l0f = floorf(lod), fl = lod - l0f, l0 = (uint32_t)l0f, l1 = min(l0 + 1, L - 1), per channel lerpf(fetch(l0), fetch(l1), fl);
 *     fetch(k) with level k's own w, h:  b = bilinear_setup(u, v, w, h);  CLAMP addressing x0 = clampi(b.i0, 0, w - 1),
 *       x1 = clampi(b.i0 + 1, 0, w - 1), rows likewise;  the four texels' channels through unorm8_to_float, then bilerp.
 *  7. a = (t.w * opacity) * fade.  If !(a > 0.0f) the decal changes nothing here -- a rule, not a shortcut: lerpf(inf, y, 0) is NaN.
 *  8. ALBEDO: alb.c = lerpf(alb.c, t.c * tint[c], a);  ROUGHNESS: rough = lerpf(rough, roughness, a);
 *     METALNESS: metal = lerpf(metal, metalness, a).
 *  9. NORMAL with normalTexture < nTextures:  m = sample(textures[normalTexture]) with the same u, v, s and texelsPerUnit;
 *     e.c = fma(m.c, 2.0f, -1.0f);  wv.c = fma(e.z, normalW[c], fma(e.y, bitangentW[c], e.x * tangentW[c]));
 *     nrm.c = lerpf(nrm.c, wv.c, a).  With no valid normal texture the flag does nothing.
 * Stores: a component of a plane is stored iff at least one decal passed step 7 at this pixel carrying its flag: ALBEDO stores
 * G1.xyz, ROUGHNESS G1.w, METALNESS G0.w, NORMAL with a valid map G2.xyz.  The stored value is in the plane's format: the float, or
 * float_to_half of it.  Every other component and every other byte keeps its bits: uncovered pixels, pixels inside no decal, rows
 * outside the call, G0.xyz, G2.w and the depth plane.
 * Known answers: a 1 x 1 opaque texel with opacity 1 and no fade puts fma(1, tint - x, x) into the albedo x inside the box; two
 * overlapping decals give different planes in either order; normalW pointing away from the surface (fade 0) changes nothing. */
#define CRYCHIC_MAX_DECALS 64
#define CRYCHIC_DECAL_MAX_TEXTURES 16
#define CRYCHIC_DECAL_ALBEDO 1u
#define CRYCHIC_DECAL_ROUGHNESS 2u
#define CRYCHIC_DECAL_METALNESS 4u
#define CRYCHIC_DECAL_NORMAL 8u
#define CRYCHIC_DECAL_NO_TEXTURE 0xFFFFFFFFu
typedef struct crychic_decal {
    float invWorld[12];                             /* world -> unit cube: q[c] = mulcol1(P.x, P.y, P.z, invWorld + 4c) */
    float boundsMin[3], boundsMax[3];               /* a world-space box around the decal (step 2) */
    float tangentW[3], bitangentW[3], normalW[3];   /* unit world directions of the cube's +x, +y, +z */
    float tint[3]; float opacity;
    float roughness, metalness;
    float fadeScale, fadeBias;                      /* angle fade; (0, 1) = none */
    float texelsPerUnit;                            /* max(texW / |edge x|, texH / |edge y|) */
    uint32_t texture, normalTexture, flags;         /* indices into the call's texture table; normalTexture 0xFFFFFFFF = none */
    uint32_t reserved;                              /* 0 */
} crychic_decal;   /* 160 bytes */
/* Fills *out from the unit cube -> world matrix `world` (the layout of crychic_instance_data.World: world.c = mulcol1(x, y, z,
 * world + 4c), world[12 .. 15] = 0 0 0 1), the decal texture's level-0 size and the cosines between which the angle fade runs
 * (fade 1 at dot(n0, normalW) >= cosFadeStart, 0 at <= cosFadeEnd).  invWorld: the inverse computed in double, rounded once; the
 * three unit axes; texelsPerUnit; fadeScale = 1 / (start - end), fadeBias = -end * fadeScale, and start == end, which only the pair
 * (1, 1) may be, means "no fade" and stores (0, 1); boundsMin / boundsMax: the box of the eight corners computed in double, widened per
 * side by 2^-10 * (that axis' extent + the largest |corner coordinate|) and rounded outwards.  It leaves tint = 1, opacity = 1,
 * roughness = metalness = 0, flags = CRYCHIC_DECAL_ALBEDO, texture = 0, normalTexture = none, reserved = 0.  Pure host code.
 * CRYCHIC_E_INVALID_ARG: a NULL argument, a non-finite or non-affine matrix, a singular one (an axis shorter than 2^-60, or a zero
 * determinant), a texture side of 0, a cosine outside [-1, 1], start < end, or start == end other than (1, 1). */
int crychic_decal_from_box(const float world[16], uint32_t texW, uint32_t texH, float cosFadeStart, float cosFadeEnd, crychic_decal* out);
/* Modifies rows [row0, row0 + rows) of the three planes in place and no other byte; reads the same rows of depth_dev (W x H, D24 in
 * the low 24 bits), the decals, the textures' texels, and View[8 .. 11] and Proj[5] of cb (a host pointer, read during the call).
 * formatFlags: the CRYCHIC_GBUFFER_G*_F16 bits, as the producers and the lighting pass take them.  textures: a HOST array of at most
 * CRYCHIC_DECAL_MAX_TEXTURES entries (device pointers inside), read during the call: it travels in the kernel's arguments, with no copy
 * and no workspace.  A pixel reads and writes only its own texels, so stitched row ranges equal the whole-frame call byte for byte,
 * for any row0 and rows, and the pass runs per strip under the multi-GPU path.  A second call blends the decals again over the first
 * call's result.  One launch on `stream`: no allocation, no synchronisation, no host read-back; capturable into a graph.
 * nDecals == 0 or rows == 0 launches nothing.
 * CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL plane or cb;
 * decals_dev NULL with nDecals > 0; textures NULL with nTextures > 0; a misaligned plane (16 bytes for a float4 plane, 8 for a half4
 * one, 4 for depth and the decals); W or H of 0; a row range outside the frame; nDecals > CRYCHIC_MAX_DECALS; nTextures >
 * CRYCHIC_DECAL_MAX_TEXTURES; a texture with a NULL pointer, a zero side or more levels than floor(log2(max(w, h))) + 1; a bit outside
 * the three format bits; a non-finite View[8 .. 11] or Proj[5], or Proj[5] == 0.  More than 2^28 pixels, or a texture of more than
 * 2^28 texels: CRYCHIC_E_UNSUPPORTED. */
int crychic_apply_decals(crychic_ctx* ctx, const crychic_pass_constants* cb, const uint32_t* depth_dev, void* g0_dev, void* g1_dev,
                         void* g2_dev, uint32_t formatFlags, const crychic_decal* decals_dev, uint32_t nDecals,
                         const crychic_texture* textures, uint32_t nTextures, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                         void* stream);

/* ---- bloom: threshold, binomial pyramid and additive composite (extension) --------------------------------
 * A pass over the finished RGBA8 frame, a separate call after the lighting pass, the fog and the depth of field and before the
 * anti-aliasing: what lies over a luma threshold is filtered down a chain of half-size levels, the chain is folded back up with a
 * scatter weight, and the result is added to the frame.  The first pass here that is a multi-resolution chain over a workspace of
 * the caller's.  A build definition: nothing of it is the reference's.  The device, a host build and the checker (tests/bloom_ref)
 * agree bit for bit.
 *
 * All arithmetic is unsigned 32-bit, divisions are integer divisions, and no intermediate reaches 2^32 (the bounds stand beside
 * each step).  Parameters: T = threshold (8-bit luma units, default 192; 0 .. 255), K = knee (default 32; 1 .. 255), r = scatter
 * (default 179; 0 .. 256), I = intensity (256 = 1.0, default 128; 0 .. 1024), n = levels (default 6;
 * 1 .. CRYCHIC_BLOOM_MAX_LEVELS), reserved (must be 0).  crychic_bloom_default_params fills the defaults (pure host code;
 * CRYCHIC_E_INVALID_ARG for NULL).
 *
 * Level sizes: W_0 = W, H_0 = H;  W_k = (W_(k-1) + 1) >> 1, H_k = (H_(k-1) + 1) >> 1 for k >= 1.  The effective level count is
 * n_eff = min(n, max(1, ceil(log2(max(W, H))))): the chain stops at the first 1 x 1 level, and a 1 x 1 frame has one level.  A
 * pyramid texel is four uint16_t: R, G, B and 0 -- 8 bytes.
 * Bright value of a frame texel (R, G, B, A):  L = 77 R + 150 G + 29 B (crychic_antialias's luma, at most 65280);  w = 0 if
 * L <= 256 T, else w = min(256, (L - 256 T) / K);  b_ch = in_ch w for R, G and B, 0 .. 255 * 256 = 65280.
 * Downsample: D_1 from b (level 0), D_(k+1) from D_k.  The filter is the 4 x 4 binomial (1, 3, 3, 1) x (1, 3, 3, 1): destination
 * (x, y) reads source columns 2x - 1 .. 2x + 2 and rows 2y - 1 .. 2y + 2, each coordinate clamped to the source level's edge,
 * sum = the 16 products (at most 64 * 65280 = 4 177 920), v = (sum + 32) >> 6, again at most 65280.
 * 2x upsample up(S)(x, y) of a level S of W_S x H_S texels:  x' = x >> 1;  xn = x' + 1 if x is odd, else x' - 1, clamped to
 * [0, W_S - 1] (x' - 1 in signed terms: it clamps to 0);  y', yn likewise from y and H_S;
 *   up = (9 S(x', y') + 3 S(xn, y') + 3 S(x', yn) + S(xn, yn) + 8) >> 4   (at most 16 * 65280 + 8, and up <= 65280).
 * Unwind:  U_(n_eff) = D_(n_eff);  for k = n_eff - 1 .. 1:  U_k = (D_k (256 - r) + up(U_(k+1)) r + 128) >> 8  (at most
 * 256 * 65280 + 128 before the shift and 65280 after it).
 * Composite, for R, G and B:  out_ch = min(255, in_ch + ((up(U_1)_ch I + 32768) >> 16))  (65280 * 1024 + 32768 < 2^27); alpha is
 * the pixel's own.
 * Known answers: (1) intensity 0 gives out == in; (2) a frame with every L <= 256 T gives out == in and every level zero; (3) a
 * frame of one colour c over the threshold has c w in every texel of every level and out_ch = min(255, c_ch + ((c_ch w I + 32768)
 * >> 16)); (4) out_ch >= in_ch always; (5) scatter 0 makes U_1 = D_1, so levels >= 2 have no influence on the frame; (6) a square
 * power-of-two frame whose input is symmetric under the eight symmetries of the square gives a symmetric output; (7) transposing any
 * input transposes the output.
 *
 * Workspace: levels 1 .. n_eff back to back, each starting on a 16-byte boundary (a level of an odd number of texels is followed by
 * 8 bytes that are never written); level k is W_k x H_k texels, row-major.  crychic_bloom_workspace_bytes is the end of level n_eff,
 * crychic_bloom_level_offset the start of level k (0 for k = 0 or k > n_eff, as for W or H of 0 or levels outside
 * 1 .. CRYCHIC_BLOOM_MAX_LEVELS); both are pure host code. */
#define CRYCHIC_BLOOM_MAX_LEVELS 8
typedef struct crychic_bloom_params {
    uint32_t threshold;
    uint32_t knee;
    uint32_t scatter;
    uint32_t intensity;
    uint32_t levels;
    uint32_t reserved[3];
} crychic_bloom_params;   /* 32 bytes */
int crychic_bloom_default_params(crychic_bloom_params* out);
size_t crychic_bloom_workspace_bytes(uint32_t W, uint32_t H, uint32_t levels);
size_t crychic_bloom_level_offset(uint32_t W, uint32_t H, uint32_t levels, uint32_t k);
/* crychic_bloom_pyramid: after it level k of workspace_dev holds U_k for k = 1 .. n_eff (the unwind runs in place over D_k); no
 * other byte of the workspace is written and in_rgba8_dev is only read.  2 n_eff - 1 launches on `stream`, one behind the other.
 * crychic_bloom_composite: rows [row0, row0 + rows) of out_rgba8_dev from the same rows of in_rgba8_dev and level 1 of the
 * workspace, and no other byte; every pixel is independent, so stitched row ranges equal the whole-frame call byte for byte;
 * rows == 0 launches nothing.  in == out exactly is allowed (in place); any other overlap is refused.  One launch.
 * crychic_bloom: the two calls above over the whole frame.
 * All three: params == NULL = the defaults; no allocation, no synchronisation, no host read-back; capturable into a graph as one
 * linear sequence of launches on `stream`.
 * CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL plane or
 * workspace; a plane that is not 4-byte aligned or a workspace that is not 16-byte aligned; W or H of 0; a row range outside the
 * frame; a parameter outside its range or a non-zero reserved word; workspace_bytes below crychic_bloom_workspace_bytes(W, H,
 * levels); a workspace (its first crychic_bloom_workspace_bytes bytes) overlapping a plane; in and out overlapping without being
 * equal.  More than 2^28 pixels: CRYCHIC_E_UNSUPPORTED. */
int crychic_bloom_pyramid(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint32_t W, uint32_t H,
                          const crychic_bloom_params* params /* NULL = defaults */, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
int crychic_bloom_composite(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H,
                            uint32_t row0, uint32_t rows, const crychic_bloom_params* params /* NULL = defaults */,
                            const void* workspace_dev, size_t workspace_bytes, void* stream);
int crychic_bloom(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H,
                  const crychic_bloom_params* params /* NULL = defaults */, void* workspace_dev, size_t workspace_bytes,
                  void* stream);

/* ---- temporal anti-aliasing: jittered frames blended into a reprojected history (extension) ---------------
 * The camera is shifted by a sub-pixel offset each frame (crychic_taa_jitter, the _jittered constant builders); crychic_taa blends
 * the finished RGBA8 frame into a history plane that it fetches through the depth plane and the previous frame's view-projection.
 * A separate call after the lighting pass and the fog and before the depth of field, the bloom and the post-process anti-aliasing:
 * the frame must still be aligned with its depth plane.  The first pass with state from one frame to the next: the caller owns two
 * history planes and swaps them.  A build definition: nothing of it is the reference's.  The device, a host build and the checker
 * (tests/taa_ref) agree bit for bit on both outputs.
 *
 * crychic_taa_jitter: sample 1 + index % 16 of the Halton (2, 3) sequence minus 0.5, in pixels, in [-0.5, 0.5).  With i = 1 + index % 16:
 * *jx = r2(i) - 0.5f, r2 the base-2 radical inverse, a multiple of 1/32: exact.  *jy = (float)n / (float)d - 0.5f with n / d the base-3
 * radical inverse of i over the denominator d = 3^k of its k digits (3, 9 or 27): one IEEE binary32 division of two exactly
 * representable integers, then one binary32 subtraction.  Pure host code; CRYCHIC_E_INVALID_ARG for a NULL pointer.
 * crychic_update_main_pass_cb_jittered / crychic_update_ssao_cb_jittered: the unjittered builders with the projection shifted so that
 * a world point which the unjittered frame shows at pixel position (x, y) is shown at (x + jx, y + jy), y growing downwards: element
 * (2, 0) of the row-vector projection becomes 0.0f + 2.0f * jx / (float)W and element (2, 1) becomes 0.0f + (-2.0f * jy) / (float)H; Proj,
 * InvProj, ViewProj, InvViewProj and ViewProjTex (ProjTex for the SSAO constants) are built from the shifted matrix by the builder's
 * own code.  jx == jy == 0 gives structures byte-identical to the unjittered builders'.  A non-finite offset: CRYCHIC_E_INVALID_ARG.
 *
 * The pass.  Float operations are IEEE binary32, each rounded once, in the order written; the named primitives are those of
 * crychic_fog above (d24_to_float, mulcol, mulcol1, rcp).  curViewProj and prevViewProj are the UNJITTERED view-projections of this
 * frame and the previous one, stored transposed like cb's matrices; cb is the frame's own (jittered) constants, of which InvViewProj
 * is read.  A history plane is W x H texels of four uint16_t (R, G, B, A), 8.8 fixed point: crychic_taa_history_bytes = W H 8.
 * Host-side constants, once per call:  sx = 2.0f / (float)W;  sy = 2.0f / (float)H;  hw = 0.5f * (float)W;  hh = 0.5f * (float)H;
 * xmax = (float)((W - 1) 256);  ymax = (float)((H - 1) 256)  (exact: W and H are at most 2^22).
 * Per pixel (px, py), with c[k], k = R, G, B, A, the four bytes of the current texel in[py W + px]:
 *   1  lo[k] = 256 min, hi[k] = 256 max of channel k = R, G, B over the 3 x 3 texels of `in` at (clamp(px + i, 0, W - 1),
 *      clamp(py + j, 0, H - 1)), i, j = -1 .. 1: clamped to the frame, not to the row range.
 *   2  d = d24_to_float(depth[py W + px]);  nx = fma((float)px + 0.5f, sx, -1.0f);  ny = fma((float)py + 0.5f, -sy, 1.0f);
 *      h[c] = mulcol(nx, ny, d, 1.0f, cb->InvViewProj + 4c), c = 0 .. 3;  rw = rcp(h[3]);  P = (h[0] rw, h[1] rw, h[2] rw).  A sky texel
 *      is no special case.
 *   3  a[c] = mulcol1(P, curViewProj + 4c), b[c] = mulcol1(P, prevViewProj + 4c), c = 0, 1, 3;  ra = rcp(a[3]);  rb = rcp(b[3]);
 *      vx = (a[0] ra - b[0] rb) hw;  vy = (b[1] rb - a[1] ra) hh  (two products, one difference, one product: four roundings each).
 *      Bitwise-equal matrices give a velocity of exactly +0 or NaN.
 *   4  fxp = ((float)px - vx) 256.0f;  fyp = ((float)py - vy) 256.0f.  The pixel HAS HISTORY iff CRYCHIC_TAA_RESET is clear and
 *      b[3] > 0 and fxp >= 0 and fxp <= xmax and fyp >= 0 and fyp <= ymax (every comparison false for NaN).  Then X = (int)floorf(fxp),
 *      xi = X >> 8, fx = X & 255, x1 = min(xi + 1, W - 1), and Y, yi, fy, y1 likewise; with t00 = history_in[yi W + xi], t10 at
 *      (x1, yi), t01 at (xi, y1), t11 at (x1, y1), per channel k = R, G, B in 32-bit unsigned arithmetic:
 *      top = t00 (256 - fx) + t10 fx;  bot = t01 (256 - fx) + t11 fx;  hv = (top (256 - fy) + bot fy + 32768) >> 16  (at most
 *      65535 2^16 + 2^15: it fits for any uint16_t content).
 *   5  hc[k] = min(max(hv[k], lo[k]), hi[k]); with CRYCHIC_TAA_NO_CLAMP hc[k] = hv[k].
 *   6  with history n[k] = (hc[k] (256 - blend) + c[k] 256 blend + 128) >> 8 (at most 65535); without, n[k] = 256 c[k].
 *   7  history_out[py W + px] = (n[R], n[G], n[B], 256 c[A]);  out[py W + px] = (min((n[k] + 128) >> 8, 255) for R, G, B;  c[A]).
 * Known answers: RESET gives out == in and history_out == 256 in.  blend == 256 gives out == in whatever the history.  Identical
 * matrices and history_in == 256 in give out == in and history_out == history_in.  A constant frame C over a constant history Hc
 * with identical matrices and NO_CLAMP: n = (Hc (256 - blend) + 256 C blend + 128) >> 8 in every texel; without NO_CLAMP hc = 256 C
 * and out == C.
 *
 * Parameters (32 bytes): blend, the weight of the current frame in 1/256 (default 26; 1 .. 256); flags (CRYCHIC_TAA_RESET: the history
 * is not read and history_in_dev may be NULL; CRYCHIC_TAA_NO_CLAMP: step 5 is skipped); reserved (must be 0).
 * crychic_taa_default_params fills the defaults (pure host code; CRYCHIC_E_INVALID_ARG for NULL).
 *
 * crychic_taa writes rows [row0, row0 + rows) of out_rgba8_dev and history_out_dev and no other byte; it reads the texels of
 * in_rgba8_dev within one row of that range, the range's rows of depth_dev and any texel of history_in_dev.  Stitched row ranges
 * therefore equal the whole-frame call byte for byte in both outputs, for any split; rows == 0 launches nothing.  params == NULL = the
 * defaults.  One launch on `stream`: no allocation, no synchronisation, no host read-back; capturable into a graph.
 * CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL plane (history_in_dev
 * only without RESET), cb or matrix; an RGBA8 or depth plane that is not 4-byte aligned or a history plane that is not 8-byte
 * aligned; W or H of 0; a row range outside the frame; a non-finite entry in cb->InvViewProj, curViewProj or prevViewProj; blend
 * outside 1 .. 256, an unknown flag bit or a non-zero reserved word; out overlapping in (the pass reads neighbours); history_out
 * overlapping history_in; a history plane overlapping in, out or depth.  More than 2^28 pixels, or W or H above 2^22 (the history
 * position in 1/256 texel is a 32-bit integer): CRYCHIC_E_UNSUPPORTED. */
#define CRYCHIC_TAA_RESET 1u
#define CRYCHIC_TAA_NO_CLAMP 2u
typedef struct crychic_taa_params {
    uint32_t blend;
    uint32_t flags;
    uint32_t reserved[6];
} crychic_taa_params;   /* 32 bytes */
int crychic_taa_jitter(uint32_t index, float* jx, float* jy);
int crychic_update_main_pass_cb_jittered(const crychic_camera* cam, uint32_t W, uint32_t H, const float shadowTransform[4][16],
                                         const float lightDirs[3][3], float jx, float jy, crychic_pass_constants* out);
int crychic_update_ssao_cb_jittered(const crychic_camera* cam, uint32_t W, uint32_t H, const float offsets[14][4], float jx, float jy,
                                    crychic_ssao_constants* out);
int crychic_taa_default_params(crychic_taa_params* out);
size_t crychic_taa_history_bytes(uint32_t W, uint32_t H);
int crychic_taa(crychic_ctx* ctx, const crychic_pass_constants* cb, const float curViewProj[16], const float prevViewProj[16],
                const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, const uint16_t* history_in_dev, uint16_t* history_out_dev,
                uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0, uint32_t rows,
                const crychic_taa_params* params /* NULL = defaults */, void* stream);

/* ---- temporal upsampling: jittered frames of the render size into a history of the display size (extension)
 * crychic_taa_upscale stands where crychic_taa stands (never both): the finished RGBA8 frame of Wi x Hi pixels, rendered with the
 * frame's jitter, is accumulated into a history of Wo x Ho texels and resolved to an RGBA8 frame of Wo x Ho pixels,
 * Wi <= Wo <= 4 Wi and Hi <= Ho <= 4 Hi, the two ratios independent.  Each output pixel weighs the current frame by how close one of
 * its samples fell to the pixel's centre, so that over the jitter sequence every output pixel is fed by samples near it.  A build
 * definition: nothing of it is the reference's.  The device, a host build and the checker (tests/taa_upscale_ref) agree bit for bit on
 * both outputs.
 *
 * Float operations, matrices, primitives and the history format are those of crychic_taa above; behind the history position
 * everything is 32-bit unsigned integer arithmetic unless said otherwise.  cb is the frame's own (jittered) constants at Wi x Hi, of
 * which InvViewProj is read; (jx, jy) is the jitter those constants were built with.
 * Host-side constants, once per call:  sx = 2.0f / (float)Wi;  sy = 2.0f / (float)Hi;  hw = 0.5f * (float)Wi;  hh = 0.5f * (float)Hi;
 * rx = (float)Wo / (float)Wi;  ry = (float)Ho / (float)Hi  (one IEEE division each);  xmax = (float)((Wo - 1) 256);
 * ymax = (float)((Ho - 1) 256);  Jx = (int)floorf(fmaf(jx, 256.0f, 0.5f));  Jy likewise from jy  (-128 .. 128).
 * Per output pixel (ox, oy):
 *   1  The pixel's centre in the input frame, in 1/256 texel, texel t's centre at 256 t:
 *      U = ((2 ox + 1) Wi 256) / (2 Wo) + Jx - 128, the division a floor division of non-negative 64-bit integers; V likewise from oy,
 *      Hi, Ho and Jy.  (The jittered frame shows at x + jx what the unjittered frame shows at x: the centre (ox + 0.5) Wi / Wo of the
 *      output pixel is found at that position plus jx, and a position p is p - 0.5 texel centres.)  ui = U >> 8 (arithmetic, -1 at
 *      the least), fu = U & 255, vi, fv likewise;  tx = clamp((U + 128) >> 8, 0, Wi - 1), ty = clamp((V + 128) >> 8, 0, Hi - 1): the
 *      NEAREST texel.
 *   2  c256[k], k = R, G, B: with t00 = in at (clamp(ui, 0, Wi - 1), clamp(vi, 0, Hi - 1)), t10 at (clamp(ui + 1), clamp(vi)), t01 at
 *      (clamp(ui), clamp(vi + 1)), t11 at (clamp(ui + 1), clamp(vi + 1)), per channel:  top = t00 (256 - fu) + t10 fu;
 *      bot = t01 (256 - fu) + t11 fu;  c256 = (top (256 - fv) + bot fv + 128) >> 8  (at most 65280).  cA = byte A of the nearest texel.
 *   3  du = min(fu, 256 - fu);  dX = min(256, (du Wo) / Wi);  dv, dY likewise from fv, Ho, Hi;  conf = ((256 - dX) (256 - dY)) >> 8;
 *      conf2 = (conf conf) >> 8;  wgt = min(256, (blend conf2) >> 8): the current frame's weight in this pixel.
 *   4  lo[k] = 256 min, hi[k] = 256 max of channel k = R, G, B over the 3 x 3 texels of `in` at (clamp(tx + i, 0, Wi - 1),
 *      clamp(ty + j, 0, Hi - 1)), i, j = -1 .. 1.
 *   5  vx, vy as steps 2 and 3 of crychic_taa give them with px = tx, py = ty, depth[ty Wi + tx] and the constants above, b[3]
 *      included: a velocity in input pixels.  fxp = ((float)ox - vx rx) 256.0f;  fyp = ((float)oy - vy ry) 256.0f  (one product, one
 *      difference, one product each).  The pixel HAS HISTORY under step 4's test of crychic_taa with these fxp, fyp, xmax and ymax and
 *      CRYCHIC_TAA_UPSCALE_RESET, and hv[k] is that step's fetch from the Wo x Ho plane history_in;  hc[k] = min(max(hv[k], lo[k]),
 *      hi[k]), with CRYCHIC_TAA_UPSCALE_NO_CLAMP hc[k] = hv[k].
 *   6  with history n[k] = (hc[k] (256 - wgt) + c256[k] wgt + 128) >> 8 (at most 65535); without, n[k] = c256[k].
 *      history_out[oy Wo + ox] = (n[R], n[G], n[B], 256 cA);  out[oy Wo + ox] = (min((n[k] + 128) >> 8, 255) for R, G, B;  cA).
 * Known answers.  RESET: history_out == c256 and out == the rounded bilinear frame.  Wo == Wi, Ho == Hi, jx == jy == 0: U = 256 ox,
 * fu = 0, c256 = 256 c, conf2 = 256, wgt = blend, rx = 1: both outputs are those of crychic_taa with the same blend and flags, byte for
 * byte.  A constant frame C over a constant history Hc with identical matrices and NO_CLAMP: n = (Hc (256 - wgt) + 256 C wgt + 128) >> 8
 * with each pixel's own wgt.  Wo == 2 Wi, Ho == 2 Hi, zero jitter: fu, fv are 64 or 192, dX = dY = 128, conf = 64, conf2 = 16 in every
 * pixel.
 *
 * Parameters (32 bytes): blend, the weight in 1/256 of a current sample that falls on the pixel's centre (default 102; 1 .. 256);
 * flags (CRYCHIC_TAA_UPSCALE_RESET, CRYCHIC_TAA_UPSCALE_NO_CLAMP: the bit values and meanings of the CRYCHIC_TAA_ flags); reserved
 * (must be 0).  crychic_taa_upscale_default_params fills the defaults (pure host code; CRYCHIC_E_INVALID_ARG for NULL).
 *
 * crychic_taa_upscale writes rows [row0, row0 + rows) of out_rgba8_dev and history_out_dev (rows of the OUTPUT) and no other byte; it
 * reads any texel of in_rgba8_dev, depth_dev and history_in_dev.  Stitched row ranges equal the whole-frame call byte for byte in both
 * outputs, for any split; rows == 0 launches nothing.  One launch on `stream`: no allocation, no synchronisation, no host read-back;
 * capturable into a graph.  CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued:
 * a NULL plane (history_in_dev only without RESET), cb or matrix; an RGBA8 or depth plane that is not 4-byte aligned or a history plane
 * that is not 8-byte aligned; a size of 0; Wo outside Wi .. 4 Wi or Ho outside Hi .. 4 Hi; a row range outside the output; a
 * non-finite matrix entry or jitter, or a jitter beyond 0.5 in magnitude; blend outside 1 .. 256, an unknown flag bit or a non-zero
 * reserved word; out overlapping in or depth; history_out overlapping history_in; a history plane overlapping in, out or depth (out
 * and the histories have Wo x Ho texels, in and depth Wi x Hi).  More than 2^28 output pixels, or Wo or Ho above 2^22: CRYCHIC_E_UNSUPPORTED. */
#define CRYCHIC_TAA_UPSCALE_RESET CRYCHIC_TAA_RESET
#define CRYCHIC_TAA_UPSCALE_NO_CLAMP CRYCHIC_TAA_NO_CLAMP
typedef struct crychic_taa_upscale_params {
    uint32_t blend;
    uint32_t flags;
    uint32_t reserved[6];
} crychic_taa_upscale_params;   /* 32 bytes */
int crychic_taa_upscale_default_params(crychic_taa_upscale_params* out);
int crychic_taa_upscale(crychic_ctx* ctx, const crychic_pass_constants* cb, const float curViewProj[16], const float prevViewProj[16],
                        float jx, float jy, const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, uint32_t Wi, uint32_t Hi,
                        const uint16_t* history_in_dev, uint16_t* history_out_dev, uint8_t* out_rgba8_dev, uint32_t Wo, uint32_t Ho,
                        uint32_t row0, uint32_t rows, const crychic_taa_upscale_params* params /* NULL = defaults */, void* stream);

/* ---- motion blur: depth-reprojected velocity, tile maximum, gather (extension) ---------------------------
 * Camera motion turned into blur of the finished RGBA8 frame.  A separate call behind the depth of field and in front of the bloom and
 * the post-process anti-aliasing; it writes a buffer of its own.  Each pixel's velocity is the reprojection of crychic_taa (steps 2
 * and 3 above) through the depth plane; each 16 x 16 tile keeps its largest velocity; each pixel gathers N samples along the largest
 * velocity of the 3 x 3 tiles around it, weighted by depth and by each side's own reach.  Camera motion only: a render item carries
 * no previous world matrix; the velocity plane is where object motion would be added.  A build definition: nothing of it is the
 * reference's.  The device, a host build and the checker (tests/motion_blur_ref) agree bit for bit on the workspace and the frame.
 *
 * Parameters (32 bytes): shutter, the exposure in 1/256 of the frame interval (default 128; 0 .. 256); samples = N (default 8; 2, 4, 8,
 * 16 or 32); maxRadius = R in pixels (default 16; 1 .. 32); flags (must be 0); reserved (must be 0).
 * crychic_motion_blur_default_params fills the defaults (pure host code; CRYCHIC_E_INVALID_ARG for NULL).
 *
 * Workspace: the velocity plane, W x H texels of two uint32_t, row-major, at offset 0; behind it, at
 * crychic_motion_blur_tile_offset(W, H) = W H 8, the tile plane, ceil(W / 16) x ceil(H / 16) uint32_t, row-major.
 * crychic_motion_blur_workspace_bytes(W, H) is the end of the tile plane.  Both are pure host code.
 *
 * Float operations are IEEE binary32, each rounded once, in the order written; the named primitives are those of crychic_fog and
 * crychic_taa (d24_to_float, mulcol, mulcol1, rcp).  curViewProj and prevViewProj are the UNJITTERED view-projections of this frame
 * and the previous one, stored transposed; of cb, InvViewProj is read.  The matrices may hold anything, NaN and infinity included.
 * Host-side constants:  sx, sy, hw, hh as in crychic_taa;  sh = (float)shutter * 0.00390625f (exact);  Rf = (float)R.
 * Step A, per pixel (px, py) of the whole frame:
 *   1  vx, vy as steps 2 and 3 of crychic_taa give them, a[3] and b[3] included.  The velocity is VALID iff a[3] > 0 and b[3] > 0
 *      and |vx| < infinity and |vy| < infinity (every comparison false for NaN); an invalid velocity is (+0, +0).
 *   2  s_x = vx sh;  s_y = vy sh  (one product each).
 *   3  m = max(|s_x|, |s_y|);  if m > Rf:  k = Rf rcp(m) (one product);  s_x = s_x k;  s_y = s_y k.
 *   4  q = clamp((int)floorf(fma(s, 16.0f, 0.5f)), -16 R, 16 R) for s = s_x, s_y: 1/16 pixel.
 *   5  velocity[py W + px] = { (uint16_t)qx | (uint32_t)(uint16_t)qy << 16,  depth[py W + px] & 0xFFFFFF }.
 * len(word) = max(|qx|, |qy|) of the two int16_t in a velocity word: the Chebyshev norm, in 1/16 pixel, at most 512.
 * key(word) = (uint64_t)len(word) << 32 | word.  Equal keys are equal words, so "the word of the largest key" is well defined.
 * Step A', per tile: tile (tx, ty) covers pixels [16 tx, 16 tx + 16) x [16 ty, 16 ty + 16) cut to the frame;
 *   tiles[ty ceil(W / 16) + tx] = the word of the largest key among the tile's velocity words.
 * Step B, per pixel (px, py) of the row range, in tile (tx, ty) = (px >> 4, py >> 4):
 *   1  vN = (nx, ny) = the word of the largest key among tiles (tx + i, ty + j), i, j = -1 .. 1, inside the tile grid.
 *   2  if len(vN) < 8:  out = in, all four bytes.
 *   3  else  b = B[py & 3][px & 3] of crychic_fog's Bayer matrix, 0 .. 15;  (wordX, dX) = velocity[py W + px];  lenX = len(wordX).
 *   4  for i = 0 .. N - 1:  m = 16 i + b - 8 N;  ox = floor((nx m + 8 N) / (16 N)), oy = floor((ny m + 8 N) / (16 N)) (floor of the
 *      exact quotient: an arithmetic shift);  dist = max(|ox|, |oy|);  the sample pixel is (clamp(px + ((ox + 8) >> 4), 0, W - 1),
 *      clamp(py + ((oy + 8) >> 4), 0, H - 1)), >> arithmetic;  (wordY, dY) is its velocity texel, lenY = len(wordY), c_i its texel
 *      of `in`;  w_i = [dY <= dX and 2 dist <= lenY] + [dY >= dX and 2 dist <= lenX]  (0, 1 or 2).
 *   5  Wt = 1 + sum w_i (at most 65);  per channel R, G, B:  S = c_X + sum w_i c_i,  out = floor((2 S + Wt) / (2 Wt)) (at most
 *      255);  alpha is the pixel's own.
 * Known answers: a still camera (bitwise-equal matrices), shutter 0 and a first frame (prev = cur) give out == in and a tile plane
 * of zeros; a pixel with velocity 0 all of whose samples lie strictly behind it keeps its bytes (a static foreground over a moving
 * background); velocities of equal length in one tile resolve to the numerically larger word.
 *
 * crychic_motion_blur_velocity: steps A and A' over the whole frame: it writes the first crychic_motion_blur_workspace_bytes(W, H)
 * bytes of the workspace and no other byte.  One launch.
 * crychic_motion_blur_gather: step B for rows [row0, row0 + rows) of out_rgba8_dev and no other byte, from in_rgba8_dev and the
 * workspace (any texel of either); stitched row ranges equal the whole-frame call byte for byte; rows == 0 launches nothing.  One
 * launch.
 * crychic_motion_blur: the two calls above over the whole frame, two launches on `stream`, one behind the other.
 * All three: params == NULL = the defaults; no allocation, no synchronisation, no host read-back; capturable into a graph.
 * CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before anything is enqueued: a NULL plane, workspace,
 * cb or matrix; a plane that is not 4-byte aligned or a workspace that is not 8-byte aligned; W or H of 0; a row range outside the
 * frame; a parameter outside its range, samples that is no power of two, non-zero flags or a non-zero reserved word; workspace_bytes
 * below crychic_motion_blur_workspace_bytes(W, H); out overlapping in (the pass gathers: it cannot run in place); the workspace (its
 * first crychic_motion_blur_workspace_bytes bytes) overlapping a plane.  More than 2^28 pixels, or W or H above 2^22:
 * CRYCHIC_E_UNSUPPORTED. */
typedef struct crychic_motion_blur_params {
    uint32_t shutter;
    uint32_t samples;
    uint32_t maxRadius;
    uint32_t flags;
    uint32_t reserved[4];
} crychic_motion_blur_params;   /* 32 bytes */
int crychic_motion_blur_default_params(crychic_motion_blur_params* out);
size_t crychic_motion_blur_workspace_bytes(uint32_t W, uint32_t H);
size_t crychic_motion_blur_tile_offset(uint32_t W, uint32_t H);
int crychic_motion_blur_velocity(crychic_ctx* ctx, const crychic_pass_constants* cb, const float curViewProj[16], const float prevViewProj[16],
                                 const uint32_t* depth_dev, uint32_t W, uint32_t H, const crychic_motion_blur_params* params /* NULL = defaults */,
                                 void* workspace_dev, size_t workspace_bytes, void* stream);
int crychic_motion_blur_gather(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0,
                               uint32_t rows, const crychic_motion_blur_params* params /* NULL = defaults */, const void* workspace_dev,
                               size_t workspace_bytes, void* stream);
int crychic_motion_blur(crychic_ctx* ctx, const crychic_pass_constants* cb, const float curViewProj[16], const float prevViewProj[16],
                        const uint32_t* depth_dev, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H,
                        const crychic_motion_blur_params* params /* NULL = defaults */, void* workspace_dev, size_t workspace_bytes,
                        void* stream);

/* ---- colour grading: a 3D look-up table, tetrahedral interpolation (extension) ----------------------------
 * The last look of the finished RGBA8 frame: every texel's (R, G, B) is looked up in a table of N x N x N colours.  A separate call
 * behind the bloom and in front of the anti-aliasing; every texel is independent, so the pass takes row ranges and may run in place.
 * A build definition: nothing of it is the reference's.  The device, a host build and the checker (tests/grade_ref) agree on every
 * byte.
 *
 * The table.  2 <= N <= CRYCHIC_GRADE_MAX_N; N^3 entries of 4 bytes; entry (i, j, k) -- i along red, j along green, k along blue,
 * the order of a .cube file -- lies at byte 4 (i + N (j + N k)).  Its bytes are R, G, B and one byte that is never looked at.
 *
 * Applying it.  All arithmetic is unsigned 32-bit, every division is the exact floor.  For a frame texel (R, G, B, A) and each of
 * its three channel values v:  p = v (N - 1);  i = min(p / 255, N - 2);  f = p - 255 i.  So 0 <= f <= 255, and v = 255 gives
 * i = N - 2 with f = 255: the last cell, at its far end.  Order the three fractions f1 >= f2 >= f3 and call their axes a1, a2, a3.
 * With V0 = (iR, iG, iB), V1 = V0 + e(a1), V2 = V1 + e(a2), V3 = V0 + (1, 1, 1) and L[V] the entry at V, for c = R, G, B:
 *   out_c = ((255 - f1) L[V0]_c + (f1 - f2) L[V1]_c + (f2 - f3) L[V2]_c + f3 L[V3]_c + 127) / 255
 * (the four weights add up to 255, so the numerator is at most 255 * 255 + 127 = 65 152), and the output's alpha is A.  Where two
 * fractions are equal the vertex that depends on their order has the weight 0: every order gives the same byte, and an
 * implementation may break ties as it likes.  Every vertex lies inside the table because i <= N - 2.
 * Known answers: a table with L(i, j, k) = (255 i, 255 j, 255 k) / (N - 1) leaves the frame as it is when N - 1 divides 255; a
 * table of N = 2 that is white at (1, 1, 1) alone gives min(R, G, B) in every channel (trilinear interpolation would give
 * R G B / 255^2).
 *
 * crychic_grade: rows [row0, row0 + rows) of out_rgba8_dev from the same rows of in_rgba8_dev and the table lut_rgba8_dev (device
 * memory, 4 N^3 bytes, only read), and no other byte; rows == 0 launches nothing.  in == out exactly is allowed (in place); any
 * other overlap is refused.  One launch on `stream`: each workgroup copies the table into 4 N^3 bytes of LDS (143 748 bytes at
 * N = 33, which the 160 KiB of a gfx950 compute unit hold) and walks the row range with a grid stride.  The planes need 4-byte
 * alignment only; where both are 16-byte aligned alike the pass moves 16 bytes per lane.  No allocation, no synchronisation, no host
 * read-back; capturable into a graph.  CRYCHIC_E_INVALID_ARG with a message, checked before the context is used and before
 * anything is enqueued: a NULL plane or table; a plane or table that is not 4-byte aligned; W or H of 0; a row range outside the
 * frame; N outside 2 .. CRYCHIC_GRADE_MAX_N; in and out overlapping without being equal; the table overlapping out.  More than 2^28
 * pixels: CRYCHIC_E_UNSUPPORTED.
 *
 * crychic_grade_build_lut (pure host code): the table of size N of an ASC CDL with a saturation, into lut_rgba8 (capacityBytes
 * >= 4 N^3; the fourth byte of every entry is 255).  Parameters: slope (default 1; 0 .. 16), offset (default 0; -4 .. 4), power
 * (default 1; 1/16 .. 16) per channel, saturation (default 1; 0 .. 4).  In binary32 with the primitives of csrc/devmath.hpp, fused
 * exactly where fma is written, for entry (iR, iG, iB) and c = R, G, B:
 *   x_c = divf(i_c, N - 1);  y_c = min(max(fma(x_c, slope_c, offset_c), 0), 1);  z_c = det_pow(y_c, power_c), and z_c = y_c where
 *   power_c == 1;  luma = fma(0.0722, z_B, fma(0.7152, z_G, 0.2126 z_R));  w_c = fma(saturation, z_c - luma, luma), and w_c = z_c
 *   where saturation == 1;  byte_c = float_to_unorm8(w_c) = (uint32_t) fma(min(max(w_c, 0), 1), 255, 0.5).
 * At y_c = 0 det_pow gives 0 whatever the power: black stays black.  The two exceptions make the defaults the identity table
 * unorm8(i / (N - 1)) byte for byte.  CRYCHIC_E_INVALID_ARG: a NULL pointer, N outside its range, a capacity below 4 N^3, a
 * parameter that is not finite or outside its range.
 *
 * crychic_load_cube_lut (pure host code): the table of an Adobe / Resolve .cube text file into lut_rgba8, *N its size; with
 * lut_rgba8 == NULL only *N is written.  Lines end in LF or CRLF and are at most 1023 bytes long.  Accepted: empty lines, lines
 * starting with '#', TITLE (ignored), DOMAIN_MIN 0 0 0, DOMAIN_MAX 1 1 1, LUT_3D_SIZE N, in any order in front of the data; then
 * exactly N^3 rows of three numbers, red fastest, each stored as float_to_unorm8 of its binary32 value (the fourth byte 255).
 * CRYCHIC_E_UNSUPPORTED: LUT_1D_SIZE, any other keyword, a domain other than 0 .. 1, N outside 2 .. CRYCHIC_GRADE_MAX_N.
 * CRYCHIC_E_INVALID_ARG: a NULL path or N, a file that cannot be read, no LUT_3D_SIZE in front of the data or two of them, too few
 * or too many rows, a number that does not parse or is not finite, a row of other than three numbers, a keyword behind the first row,
 * a line longer than 1023 bytes or holding a NUL byte, a capacity below 4 N^3.  A line that starts with a letter is a keyword line: a
 * row that starts with "nan" or "inf" is refused as an unknown keyword. */
#define CRYCHIC_GRADE_MAX_N 33
typedef struct crychic_grade_params {
    float slope[3];
    float offset[3];
    float power[3];
    float saturation;
} crychic_grade_params;   /* 40 bytes */
int crychic_grade_default_params(crychic_grade_params* out);
int crychic_grade_build_lut(const crychic_grade_params* params /* NULL = defaults */, uint32_t N, uint8_t* lut_rgba8, size_t capacityBytes);
int crychic_load_cube_lut(const char* path, uint8_t* lut_rgba8, size_t capacityBytes, uint32_t* N);
int crychic_grade(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0,
                  uint32_t rows, const uint8_t* lut_rgba8_dev, uint32_t N, void* stream);

/* ---- sharpening: a contrast-adaptive negative-lobe cross filter (extension) -----------------------------------
 * What the temporal passes' bilinear history fetch softened, put back: a separate call directly behind crychic_taa or
 * crychic_taa_upscale and in front of the depth of field.  A build definition: nothing of it is the reference's.  It uses 32-bit
 * integers only, every division is the exact floor of non-negative operands; the device, a host build, the checker
 * (tests/sharpen_ref) and a numpy restatement agree on every byte.
 *
 * For the pixel e at (x, y) the neighbours are b = (x, y - 1), d = (x - 1, y), f = (x + 1, y), h = (x, y + 1), their coordinates
 * clamped to the frame [0, W - 1] x [0, H - 1] -- not to the row range of the call.  Per channel c = R, G, B on the bytes:
 *   mn_c = min(b, d, e, f, h)      mx_c = max(b, d, e, f, h)
 *   q_c  = min( mx_c == 0   ? 0 : (mn_c << 12) / mx_c,
 *               mn_c == 255 ? 0 : ((255 - mx_c) << 12) / (255 - mn_c) )
 *   a    = min(q_R, q_G, q_B, limit)
 *   t    = (a * strength) >> 8
 *   S_c  = b_c + d_c + f_c + h_c
 *   num_c = 16384 * e_c - t * S_c          den = 4 * (4096 - t)
 *   out_c = (num_c + den / 2) / den        out_A = e_A
 * This is the filter (e - w S) / (1 - 4 w) with one weight w = t / 16384 for the three channels; the limiter q holds w to what the
 * local minimum and maximum leave room for, so num_c >= 0 and out_c <= 255 always and the definition has no clamp.  Known answers:
 * strength 0 or limit 0 return the input's bytes; so does a flat neighbourhood at any strength, and a pixel with a 0 or a 255 in
 * the cross of any of its channels (that channel's q is 0); a centre of 200 in a ring of 100 at strength 256 and the default limit gives
 * q = 1453, t = 1453 and 255 in each channel.
 *
 * Parameters: strength 0 .. CRYCHIC_SHARPEN_MAX_STRENGTH (256: the whole of the limited weight), limit 0 ..
 * CRYCHIC_SHARPEN_MAX_LIMIT (Q12; the default 3072 is 4 w <= 0.75, that is w <= 0.1875), two reserved words that must be 0.
 * crychic_sharpen_default_params: strength CRYCHIC_SHARPEN_DEFAULT_STRENGTH -- what tests/sharpen_quality.py measured
 * (profiles/sharpen_quality.txt) --, limit 3072.
 *
 * crychic_sharpen: rows [row0, row0 + rows) of out_rgba8_dev from in_rgba8_dev (rows row0 - 1 .. row0 + rows of it, clamped), and no
 * other byte; rows == 0 launches nothing; ranges stitch to the whole-frame result.  One launch on `stream`, no LDS: where W is a
 * multiple of 4 and both planes are 16-byte aligned a lane moves 16 bytes per load and store and takes the pixels beside its four
 * from the neighbouring lanes; any other width or 4-byte alignment takes a slower kernel of one pixel per lane and is never refused.
 * No allocation, no synchronisation, no host read-back; capturable into a graph.  CRYCHIC_E_INVALID_ARG with a message, checked
 * before the context is used and before anything is enqueued: a NULL plane; a plane that is not 4-byte aligned; W or H of 0; a row
 * range outside the frame; strength or limit outside its range; a reserved word that is not 0; in and out overlapping in any way
 * (the pass reads neighbours: it cannot run in place).  More than 2^28 pixels: CRYCHIC_E_UNSUPPORTED. */
#define CRYCHIC_SHARPEN_MAX_STRENGTH 256
#define CRYCHIC_SHARPEN_MAX_LIMIT 3584
#define CRYCHIC_SHARPEN_DEFAULT_STRENGTH 96
#define CRYCHIC_SHARPEN_DEFAULT_LIMIT 3072
typedef struct crychic_sharpen_params {
    uint32_t strength;
    uint32_t limit;
    uint32_t reserved[2];
} crychic_sharpen_params;   /* 16 bytes */
int crychic_sharpen_default_params(crychic_sharpen_params* out);
int crychic_sharpen(crychic_ctx* ctx, const uint8_t* in_rgba8_dev, uint8_t* out_rgba8_dev, uint32_t W, uint32_t H, uint32_t row0,
                    uint32_t rows, const crychic_sharpen_params* params /* NULL = defaults */, void* stream);

/* ---- multi-GPU strip plan (pure host arithmetic) ---------------------------------------------- */
/* Full-res rows [*row0, *row0 + *rows) owned by `rank` of `nranks` for an H-row frame: strips are multiples
 * of 2 rows (half-res alignment); the last rank takes the remainder. */
int crychic_strip_rows(uint32_t H, int nranks, int rank, uint32_t* row0, uint32_t* rows);

/* ---- multi-GPU exchange (SURVEY.md 8b `crychic_allgather_frame`, 8e): RCCL over xGMI ----------------------------- */
/* The reference is single-GPU (NodeMask 0, CRYCHIC.cpp:96,105); these entry points complete the back buffer that
 * CRYCHIC::Draw presents (CRYCHIC.cpp:282-297) when N GPUs each render a row strip of it.  One communicator per GPU.
 * Every rank renders its strip IN PLACE into a full W x H RGBA8 frame buffer; the exchange fills in the peers' strips,
 * stream-ordered behind the strip's lighting pass, with no host synchronisation.  Any RCCL failure returns
 * CRYCHIC_E_COMM (crychic_last_error() carries RCCL's own message). */
typedef struct crychic_comm crychic_comm;
#define CRYCHIC_COMM_ID_BYTES 128

/* One process per GPU: rank 0 obtains a rendezvous id (ncclGetUniqueId), hands it to its peers out of band (file, socket,
 * key-value store), then every rank calls crychic_comm_create (ncclCommInitRank: blocks until all nranks have joined). */
int crychic_comm_unique_id(uint8_t id[CRYCHIC_COMM_ID_BYTES]);
int crychic_comm_create(crychic_ctx* ctx, int nranks, int rank, const uint8_t id[CRYCHIC_COMM_ID_BYTES], crychic_comm** out);
/* One process driving all GPUs (the reference's own shape: one WinMain, one thread): communicators for ctxs[0..nranks),
 * rank k on ctxs[k]'s device (ncclCommInitAll). */
int crychic_comm_create_all(crychic_ctx* const* ctxs, int nranks, crychic_comm** out);
void crychic_comm_destroy(crychic_comm* comm);
/* Tears the communicator down without waiting for outstanding operations (ncclCommAbort): the way out of an exchange a
 * peer never joined.  The handle stays valid only for crychic_comm_destroy. */
int crychic_comm_abort(crychic_comm* comm);
int crychic_comm_rank(const crychic_comm* comm);
int crychic_comm_size(const crychic_comm* comm);
/* 0 while no asynchronous RCCL error is pending on the communicator, else CRYCHIC_E_COMM. */
int crychic_comm_async_error(crychic_comm* comm);

/* All-gather of the composed strips.  bounds = NULL: the crychic_strip_rows plan; otherwise nranks x (row0, rows) pairs that
 * tile the frame in rank order (any heights: cost-balanced strips).  Equal strips run as one in-place ncclAllGather, ragged
 * ones as one group of in-place ncclBroadcasts (one per strip).  Must be called by every rank, in the same order. */
int crychic_allgather_frame(crychic_comm* comm, uint8_t* frame_rgba8_dev, uint32_t W, uint32_t H, const uint32_t* bounds,
                            void* stream);
/* The same for a single host thread that owns every rank: frames_rgba8_dev[k] / streams[k] belong to comms[k]. */
int crychic_allgather_frame_all(crychic_comm* const* comms, int nranks, uint8_t* const* frames_rgba8_dev, uint32_t W, uint32_t H,
                                const uint32_t* bounds, void* const* streams);
/* SURVEY.md 8e "overlap by chunking the strip and gathering on a side stream": crychic_draw_hot_path for this rank's strip
 * (frame->row0 / rows must be this rank's entry of the plan, frame->out_rgba8_dev the full W x H frame) AND the exchange, with the
 * lighting pass issued in `nparts` (1 .. CRYCHIC_MAX_EXCHANGE_PARTS) consecutive row ranges: as soon as range p is lit, range p of
 * every rank's strip travels (one group of in-place ncclBroadcasts on a stream the communicator owns) while the caller's stream
 * lights range p + 1.  Ranges are whole half-res rows -- the crychic_strip_rows cut of each strip's rows -- so the image is the
 * one crychic_draw_hot_path + crychic_allgather_frame produce, bit for bit.  On return the caller's stream is ordered behind the last
 * range's exchange (no host wait).  nparts == 1 is exactly those two calls on the caller's stream.  Every rank must call it with
 * the same bounds and nparts, in the same order relative to the communicator's other collectives.  One process per GPU only. */
#define CRYCHIC_MAX_EXCHANGE_PARTS 8
int crychic_draw_hot_path_shared(crychic_comm* comm, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                                 const crychic_frame_desc* frame, const uint32_t* bounds, uint32_t nparts, void* stream);
/* The same with spot lights (crychic_draw_hot_path_spots); numSpotLights == 0 is crychic_draw_hot_path_shared. */
int crychic_draw_hot_path_shared_spots(crychic_comm* comm, const crychic_ssao_constants* ssaoCB, const crychic_pass_constants* passCB,
                                       const crychic_frame_desc* frame, const uint32_t* bounds, uint32_t nparts,
                                       const crychic_light* spot_lights_dev, uint32_t numSpotLights, void* stream);
/* The same with shadowed spot lights (crychic_draw_hot_path_spots_shadowed): each rank binds the maps it rendered. */
int crychic_draw_hot_path_shared_spots_shadowed(crychic_comm* comm, const crychic_ssao_constants* ssaoCB,
                                                const crychic_pass_constants* passCB, const crychic_frame_desc* frame,
                                                const uint32_t* bounds, uint32_t nparts, const crychic_light* spot_lights_dev,
                                                uint32_t numSpotLights, const crychic_spot_shadows* spotShadows, void* stream);
/* The same with shadowed point lights (crychic_draw_hot_path_point_shadows): each rank binds the faces it rendered. */
int crychic_draw_hot_path_shared_point_shadows(crychic_comm* comm, const crychic_ssao_constants* ssaoCB,
                                               const crychic_pass_constants* passCB, const crychic_frame_desc* frame,
                                               const uint32_t* bounds, uint32_t nparts, const crychic_light* spot_lights_dev,
                                               uint32_t numSpotLights, const crychic_spot_shadows* spotShadows,
                                               const crychic_point_shadows* pointShadows, void* stream);
/* Stream-ordered rendezvous of all ranks (a one-word ncclAllReduce): brackets timed regions; no host wait inside. */
int crychic_comm_barrier(crychic_comm* comm, void* stream);

#ifdef __cplusplus
}
#endif
#endif
