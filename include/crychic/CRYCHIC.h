// CRYCHIC.h -- headless counterpart of the reference application class (CRYCHIC.h:56-190, CRYCHIC.cpp) for the
// deferred hot path: same member names (mSsao, mDeferred, mShadowMap, mMainPassCB, mFrameResources ...), same
// Initialize / OnResize / Update / Draw call sequence, D3D12 replaced by libcrychic_hip.so.
//
// What Draw() covers: the whole deferred branch of CRYCHIC::Draw -- DrawSceneToShadowMap, DrawNormalsAndDepth
// (CRYCHIC.cpp:208,214), ComputeSsao (:220-221), DrawGBuffer (:236) and the deferred lighting + sky (:238-279) -- on
// the reference's live scene (100 instanced boxes + grid, CRYCHIC.cpp:2274-2436).  Set mRunProducerPasses = false to
// feed externally produced planes through the Resource accessors instead.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>
#include "DeferredShading.h"
#include "FrameResource.h"
#include "ShadowMap.h"
#include "Ssao.h"

const int gNumFrameResources = 3;  // CRYCHIC.h:20

class GameTimer {  // Common/GameTimer.h: only what Update/Draw read
public:
    float TotalTime() const { return mTotal; }
    float DeltaTime() const { return mDelta; }
    void Tick(float dt) { mDelta = dt; mTotal += dt; }
private:
    float mTotal = 0.0f, mDelta = 0.0f;
};

class Camera {  // Common/Camera.h:20-97: position / look / up state; the matrices are rebuilt from it by the C ABI's builders
public:
    void SetPosition(float x, float y, float z) { mCam.pos[0] = x; mCam.pos[1] = y; mCam.pos[2] = z; }
    void SetLens(float fovY, float aspect, float zn, float zf) { mCam.fovY = fovY; mCam.aspect = aspect; mCam.nearZ = zn; mCam.farZ = zf; }
    void LookTo(float lx, float ly, float lz, float ux, float uy, float uz) { mCam.look[0] = lx; mCam.look[1] = ly; mCam.look[2] = lz; mCam.up[0] = ux; mCam.up[1] = uy; mCam.up[2] = uz; }
    void LookAt(const DirectX::XMFLOAT3& pos, const DirectX::XMFLOAT3& target, const DirectX::XMFLOAT3& up)   // Camera.cpp:131-154
    {
        SetPosition(pos.x, pos.y, pos.z);
        LookTo(target.x - pos.x, target.y - pos.y, target.z - pos.z, up.x, up.y, up.z);
        UpdateViewMatrix();
    }
    DirectX::XMFLOAT3 GetPosition3f() const { return { mCam.pos[0], mCam.pos[1], mCam.pos[2] }; }
    DirectX::XMFLOAT3 GetLook3f() const { return { mCam.look[0], mCam.look[1], mCam.look[2] }; }
    DirectX::XMFLOAT3 GetUp3f() const { return { mCam.up[0], mCam.up[1], mCam.up[2] }; }
    DirectX::XMFLOAT3 GetRight3f() const { float r[3]; Cross(mCam.up, mCam.look, r); Normalize(r); return { r[0], r[1], r[2] }; }
    void Walk(float d) { for (int i = 0; i < 3; ++i) mCam.pos[i] += d * mCam.look[i]; }                    // Camera.cpp:190-199
    void Strafe(float d) { float r[3]; Cross(mCam.up, mCam.look, r); Normalize(r); for (int i = 0; i < 3; ++i) mCam.pos[i] += d * r[i]; }  // :179-188
    void Pitch(float angle)                                                                                // :201-211, about the right vector
    {
        float r[3]; Cross(mCam.up, mCam.look, r); Normalize(r);
        Rotate(mCam.up, r, angle); Rotate(mCam.look, r, angle);
    }
    void RotateY(float angle)                                                                              // :213-224, about the world y axis
    {
        const float y[3] = { 0.0f, 1.0f, 0.0f };
        Rotate(mCam.up, y, angle); Rotate(mCam.look, y, angle);
    }
    void UpdateViewMatrix()                                                                                // :226-273: re-orthonormalise
    {
        float r[3], u[3];
        Normalize(mCam.look);
        Cross(mCam.up, mCam.look, r); Normalize(r);
        Cross(mCam.look, r, u); Normalize(u);
        for (int i = 0; i < 3; ++i) mCam.up[i] = u[i];
    }
    float GetNearZ() const { return mCam.nearZ; }
    float GetFarZ() const { return mCam.farZ; }
    float GetFovY() const { return mCam.fovY; }
    float GetAspect() const { return mCam.aspect; }
    const crychic_camera& Raw() const { return mCam; }
private:
    static void Cross(const float a[3], const float b[3], float o[3]) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
    static void Normalize(float v[3]) { const float l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= l; v[1] /= l; v[2] /= l; }
    static void Rotate(float v[3], const float axis[3], float angle)   // Rodrigues; left-handed like XMMatrixRotationAxis (clockwise looking along the axis towards the origin)
    {
        const float c = std::cos(angle), s = std::sin(angle);
        float k[3]; Cross(axis, v, k);
        const float d = (axis[0] * v[0] + axis[1] * v[1] + axis[2] * v[2]) * (1.0f - c);
        for (int i = 0; i < 3; ++i) v[i] = v[i] * c + k[i] * s + axis[i] * d;
    }
    crychic_camera mCam = { { 0, 0, 0 }, { 0, 0, 1 }, { 0, 1, 0 }, 0.7853981634f, 1.0f, 1.0f, 1000.0f };
};

// Common/d3dUtil.h:163-214 (the fields the draws consume)
struct BoundingBox { DirectX::XMFLOAT3 Center = { 0, 0, 0 }, Extents = { 1, 1, 1 }; };   // DirectXCollision's, as far as the culling needs it
struct SubmeshGeometry {
    UINT IndexCount = 0;
    UINT StartIndexLocation = 0;
    int BaseVertexLocation = 0;
    BoundingBox Bounds;
};
struct MeshGeometry {
    std::string Name;
    std::unique_ptr<ID3D12Resource> VertexBufferGPU, IndexBufferGPU;
    UINT VertexCount = 0, IndexCount = 0;
    std::unordered_map<std::string, SubmeshGeometry> DrawArgs;
};
// Common/d3dUtil.h:240-265
struct Material {
    std::string Name;
    int MatCBIndex = -1;
    int DiffuseSrvHeapIndex = -1;
    int NormalSrvHeapIndex = -1;
    int NumFramesDirty = gNumFrameResources;
    DirectX::XMFLOAT4 DiffuseAlbedo = { 1.0f, 1.0f, 1.0f, 1.0f };
    DirectX::XMFLOAT3 FresnelR0 = { 0.01f, 0.01f, 0.01f };
    float Roughness = .25f;
    DirectX::XMFLOAT4X4 MatTransform = crychic_detail::Identity4x4();
};
// CRYCHIC.h:23-42
struct RenderItem {
    RenderItem() = default;
    RenderItem(const RenderItem& rhs) = delete;
    Material* Mat = nullptr;
    MeshGeometry* Geo = nullptr;
    UINT IndexCount = 0;
    UINT StartIndexLocation = 0;
    int BaseVertexLocation = 0;
    UINT InstanceCount = 0;
    std::vector<InstanceData> Instances;
    UINT itemIndex = 0;
    BoundingBox Bounds;
};
enum class RenderLayer : int { Opaque = 0, OpaqueShadow, Count };  // CRYCHIC.h:44-54 (the layers the deferred path draws)

class CRYCHIC {
public:
    CRYCHIC(int deviceOrdinal, UINT width, UINT height) : mClientWidth(width), mClientHeight(height)
    {
        mDeviceOrdinal = deviceOrdinal;
        md3dDevice = std::make_unique<ID3D12Device>(deviceOrdinal);
        mCommandList = std::make_unique<ID3D12GraphicsCommandList>();
    }
    CRYCHIC(const CRYCHIC& rhs) = delete;
    CRYCHIC& operator=(const CRYCHIC& rhs) = delete;
    ~CRYCHIC()
    {
        if (mCommandList) { try { mCommandList->Flush(); } catch (...) {} }
        if (mComm) crychic_comm_destroy(mComm);
        for (auto& fr : mFrameResources) if (fr && fr->FenceEvent) (void)hipEventDestroy(fr->FenceEvent);
    }

    bool Initialize()  // CRYCHIC.cpp:38-86
    {
        mCamera.SetPosition(0.0f, 2.0f, -15.0f);                                                   // :46
        mShadowMap = std::make_unique<ShadowMap>(md3dDevice.get(), mShadowMapSize, mShadowMapSize); // :48-49
        mSsao = std::make_unique<Ssao>(md3dDevice.get(), mCommandList.get(), mClientWidth, mClientHeight);  // :51-54
        mDeferred = std::make_unique<DeferredShading>(md3dDevice.get(), mClientWidth, mClientHeight, DXGI_FORMAT_R32G32B32A32_FLOAT);  // :56-58
        BuildShapeGeometry();                                                                       // :65
        BuildMaterials();                                                                           // :67
        BuildCascadeShadowRenderItems();                                                            // :70
        BuildCascadeShadowRenderItemsWithShadow();                                                  // :71
        BuildFrameResources();                                                                      // :72
        OnResize();
        mCommandList->Flush();                                                                      // :83
        return true;
    }

    void OnResize()  // CRYCHIC.cpp:110-128 (+ D3DApp::OnResize's back/depth buffer re-creation)
    {
        const size_t n = (size_t)mClientWidth * mClientHeight;
        mDepthStencilBuffer = FramePlane();
        CrychicHipThrowIfFailed(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(mDepthStencilBuffer->Data()), 0x00FFFFFF, n));
        mBackBuffer = FramePlane();
        if (mAntiAliasing) mBackBufferAA = FinalPlane();
        if (mDepthOfField) mBackBufferDoF = FramePlane();
        if (mScreenSpaceReflections) mBackBufferSSR = FramePlane();
        if (mSsrGloss) AllocateSsrPyramid();
        if (mBloom) AllocateBloom();
        if (mColourGrade) mBackBufferGrade = FinalPlane();
        if (mSharpening) mBackBufferSharp = FinalPlane();
        if (mTemporalAA) AllocateTemporalAA();                                                      // new history planes: the next frame is a reset frame
        if (mMotionBlur) AllocateMotionBlur();                                                      // the next frame counts as the first: no previous camera
        if (mTemporalUpscale) AllocateTemporalUpscale();                                            // the display size stays; the next frame is a reset frame
        mCamera.SetLens(0.25f * 3.1415926535f, AspectRatio(), 1.0f, 100.0f);                       // :114
        if (mSsao) { mSsao->OnResize(mClientWidth, mClientHeight); mSsao->RebuildDescriptors(mDepthStencilBuffer.get()); }
        if (mDeferred) { mDeferred->OnResize(mClientWidth, mClientHeight); mDeferred->BuildDescriptors(); }
    }
    void Resize(UINT w, UINT h) { mClientWidth = w; mClientHeight = h; OnResize(); }
    // The G-buffer planes' formats (DeferredShading.h): re-creates mDeferred, its contents are lost as on a resize.  The default is
    // the reference's, R32G32B32A32_FLOAT for all three; DrawGBuffer and Draw pass the formats on.
    void SetGBufferFormat(DXGI_FORMAT g0, DXGI_FORMAT g1, DXGI_FORMAT g2)
    {
        const DXGI_FORMAT formats[3] = { g0, g1, g2 };
        mCommandList->Flush();
        mDeferred = std::make_unique<DeferredShading>(md3dDevice.get(), mClientWidth, mClientHeight, formats);
        mDeferred->BuildDescriptors();
    }

    void Update(const GameTimer& gt)  // CRYCHIC.cpp:130-170
    {
        mCurrFrameResourceIndex = (mCurrFrameResourceIndex + 1) % gNumFrameResources;
        mCurrFrameResource = mFrameResources[mCurrFrameResourceIndex].get();
        // :138-146: wait until the GPU has finished the frame that last used this resource
        if (mCurrFrameResource->Fence != 0) CrychicHipThrowIfFailed(hipEventSynchronize(mCurrFrameResource->FenceEvent));
        mLightRotationAngle += 0.0f * gt.DeltaTime();                                               // :152
        const float c = std::cos(mLightRotationAngle), s = std::sin(mLightRotationAngle);
        for (int i = 0; i < 3; ++i) {                                                               // :154-160 (XMMatrixRotationY)
            const DirectX::XMFLOAT3 d = mBaseLightDirections[i];
            mRotatedLightDirections[i] = { d.x * c + d.z * s, d.y, -d.x * s + d.z * c };
        }
        mLastTimer = gt;                                                                            // CaptureEnvironment's TotalTime
        UpdateInstanceData(gt);                                                                     // :164
        UpdateMaterialBuffer(gt);                                                                   // :165
        UpdateCascadeShadowTransform(gt);
        UpdateSpotShadowTransforms();
        UpdatePointShadowTransforms();
        if (mTemporalAA || mTemporalUpscale) CrychicThrowIfFailed(crychic_taa_jitter(mTaaFrameIndex++, &mTaaJitter[0], &mTaaJitter[1]));   // this frame's sub-pixel offset
        UpdateMainPassCB(gt);
        UpdateShadowPassCB(gt);
        UpdateSsaoCB(gt);
    }

    void Draw(const GameTimer&)  // CRYCHIC.cpp:172-306, deferred branch
    {
        if ((!mWholeFrame || mComm) && (mAntiAliasing || mFog || mDepthOfField || mBloom || mTemporalAA || mMotionBlur || mScreenSpaceReflections || mTemporalUpscale || mColourGrade || mSharpening)) {
            const char* pass = mAntiAliasing ? "anti-aliasing" : mFog ? "fog" : mDepthOfField ? "depth of field" : mBloom ? "bloom"
                             : mTemporalAA ? "temporal anti-aliasing" : mMotionBlur ? "motion blur" : mScreenSpaceReflections ? "screen-space reflections"
                             : mTemporalUpscale ? "temporal upsampling" : mColourGrade ? "colour grade" : "sharpening";
            throw CrychicException(CRYCHIC_E_INVALID_ARG, std::string("CRYCHIC::Draw (") + pass + " takes the whole frame on one GPU: no SetStrip / JoinNode)",
                                   __FILE__, __LINE__);
        }
        if (mSsrGloss && !mScreenSpaceReflections)
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::Draw (SetScreenSpaceReflectionGloss is on and SetScreenSpaceReflections is not)", __FILE__,
                                   __LINE__);
        if (mTemporalUpscale && (mTemporalAA || mDepthOfField || mMotionBlur))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, std::string("CRYCHIC::Draw (temporal upsampling together with ") +
                                   (mTemporalAA ? "temporal anti-aliasing: one temporal pass resolves a frame)"
                                    : mDepthOfField ? "depth of field: the pass reads a depth plane of the frame's size)"
                                    : "motion blur: the pass reads a depth plane of the frame's size)"), __FILE__, __LINE__);
        if (mRunProducerPasses) {
            DrawSceneToShadowMap();                                                                 // :208
            if (mFuseCameraPasses) DrawNormalsDepthAndGBuffer();                                    // :214 + :236 on one rasterisation
            else { DrawNormalsAndDepth(); DrawGBuffer(); }
            if (mDecalCount) ApplyDecals();                                                         // SetDecals: into the fresh G-buffer
        }
        if (mFollowSun && !mOwner) FollowSun();                                                     // SetProceduralSky: the sky under this frame's sun
        // L: whose cube map, local lights and local-light shadow maps this frame reads -- a capture's probe reads its owner's
        const CRYCHIC& L = mOwner ? *mOwner : *this;
        crychic_frame_desc f = {};
        f.W = mClientWidth; f.H = mClientHeight;
        f.blurCount = mBlurCount;                                                                   // :221
        f.numDirLights = mNumDirLights;
        f.pcfSearchRadius = crychic_pcf_search_radius(mShadowMap->Width(), mPcfLiteral ? 1 : 0);
        f.flags = (mSkyEnabled ? CRYCHIC_LIGHT_SKY : 0u) | (L.mCubeMapLevels > 1 ? CRYCHIC_LIGHT_CUBE_LEVELS(L.mCubeMapLevels) : 0u);   // :278-279, :1148-1151
        if (L.mGlossyReflections && L.mCubeMapLevels > 1) f.flags |= CRYCHIC_LIGHT_CUBE_GLOSS;      // the level from the pixel's roughness
        if (L.mCubeMapHasTail) f.flags |= CRYCHIC_LIGHT_AMBIENT_SH;                                 // the ambient colour from the environment tail
        if (L.mCubeMapHasTable && (f.flags & CRYCHIC_LIGHT_CUBE_GLOSS)) f.flags |= CRYCHIC_LIGHT_ENV_BRDF;   // the reflection weighed by the table behind it
        if (L.mCubeMapHasProbe && L.mProbeBoxSet && (f.flags & CRYCHIC_LIGHT_CUBE_GLOSS)) f.flags |= CRYCHIC_LIGHT_CUBE_PARALLAX;   // the lookup box-projected through the probe volume in its tail
        f.flags |= mDeferred->FormatFlags();                                                        // a half4 plane: its CRYCHIC_GBUFFER_G*_F16 bit
        f.row0 = mStripRow0; f.rows = mWholeFrame ? mClientHeight : mStripRows;                      // whole frame unless SetStrip / JoinNode
        f.normal_dev = mSsao->NormalMap()->Data();
        f.depth_dev = static_cast<const uint32_t*>(mDepthStencilBuffer->Data());
        f.randvec_dev = static_cast<const uint8_t*>(mSsao->RandomVectorMap()->Data());
        f.g0_dev = static_cast<const float*>(mDeferred->Resource(0)->Data());
        f.g1_dev = static_cast<const float*>(mDeferred->Resource(1)->Data());
        f.g2_dev = static_cast<const float*>(mDeferred->Resource(2)->Data());
        for (int i = 0; i < 4; ++i) f.shadow_dev[i] = static_cast<const uint32_t*>(mShadowMap->Resource(i)->Data());
        f.shadowDim = mShadowMap->Width();
        if (!L.mCubeMap) throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::Draw (no cube map set)", __FILE__, __LINE__);
        f.cube_dev = static_cast<const uint8_t*>(L.mCubeMap->Data());
        f.cubeDim = L.mCubeMapSize;
        f.ambient0_dev = static_cast<uint16_t*>(mSsao->AmbientMap()->Data());
        f.ambient1_dev = static_cast<uint16_t*>(mSsao->AmbientMap1()->Data());
        f.edge_dev = mSsao->EdgePlane()->Data();
        f.out_rgba8_dev = mRenderTarget ? mRenderTarget : static_cast<uint8_t*>(mBackBuffer->Data());   // mRenderTarget: a capture's face
        const SsaoConstants& scb = mCurrFrameResource->SsaoCB->Element(0);
        const PassConstants& pcb = mCurrFrameResource->PassCB->Element(0);
        // Several GPUs, one frame: the peers' strips arrive in place behind this strip's lighting pass (RCCL over xGMI), so the
        // back buffer that Present sees is complete on every GPU.  The reference has one GPU (NodeMask 0, CRYCHIC.cpp:96,105).
        // With SetExchangeParts(n > 1) the lighting pass runs in n row ranges and each range travels while the next is lit.
        // Local lights (SetLocalLights; an extension the reference's shader leaves dead): point lights ride in the frame descriptor,
        // spot lights and both kinds of shadow take the _point_shadows entries.  With no spot lights, or a shadow count of 0, those
        // entries are the narrower ones bit for bit (include/crychic_hip.h).
        if (L.mPointLights) { f.point_lights_dev = static_cast<const crychic_light*>(L.mPointLights->Data()); f.numPointLights = L.mNumPointLights; }
        const crychic_light* spots = L.mSpotLights ? static_cast<const crychic_light*>(L.mSpotLights->Data()) : nullptr;
        // Shadowed spot lights (SetSpotShadows): the first mSpotShadowCount spot lights read their maps through ShadowTransforms[4 + k]
        crychic_spot_shadows sh = {};
        sh.count = spots ? L.mSpotShadowCount : 0u;
        sh.dim = L.mSpotShadowDim;
        for (uint32_t k = 0; k < sh.count; ++k) sh.maps[k] = static_cast<const uint32_t*>(L.mSpotShadowMaps[k]->Data());
        const auto* ssaoCB = reinterpret_cast<const crychic_ssao_constants*>(&scb);
        const auto* passCB = reinterpret_cast<const crychic_pass_constants*>(&pcb);
        // Shadowed point lights (SetPointShadows): the first mPointShadowCount point lights read their six faces through shadowProj
        crychic_point_shadows psh = {};
        psh.count = L.mPointShadowCount;
        psh.dim = L.mPointShadowDim;
        for (uint32_t k = 0; k < psh.count; ++k) {
            psh.maps[k] = static_cast<const uint32_t*>(L.mPointShadowMaps[k]->Data());
            std::memcpy(psh.shadowProj[k], L.mPointShadowProjs[k], sizeof psh.shadowProj[k]);
        }
        if (mComm)
            CrychicThrowIfFailed(crychic_draw_hot_path_shared_point_shadows(mComm, ssaoCB, passCB, &f, mStripBounds.empty() ? nullptr : mStripBounds.data(),
                                                                            mExchangeParts, spots, L.mNumSpotLights, &sh, &psh, mCommandList->Stream()));
        else
            CrychicThrowIfFailed(crychic_draw_hot_path_point_shadows(md3dDevice->Ctx(), ssaoCB, passCB, &f, spots, L.mNumSpotLights, &sh, &psh,
                                                                     mCommandList->Stream()));
        // The passes behind the lighting pass, in the chain's order (the comment above SetAntiAliasing).  `frame` is what the next
        // stage reads: the fog works in place on it, every other stage writes a buffer of its own and hands that on.
        uint8_t* frame = f.out_rgba8_dev;
        auto bytes = [](const std::unique_ptr<ID3D12Resource>& r) { return static_cast<uint8_t*>(r->Data()); };
        if (mScreenSpaceReflections && mSsrGloss) {         // the glossy variant: the lit frame's pyramid, then the pass that reads it
            CrychicThrowIfFailed(crychic_ssr_pyramid(md3dDevice->Ctx(), frame, mClientWidth, mClientHeight, mSsrGlossParams.levels, mSsrPyramid->Data(),
                                                     mSsrPyramid->Bytes(), mCommandList->Stream()));
            CrychicThrowIfFailed(crychic_ssr_glossy(md3dDevice->Ctx(), passCB, f.g0_dev, f.g1_dev, f.g2_dev, f.depth_dev, frame, mSsrPyramid->Data(),
                                                    mSsrPyramid->Bytes(), bytes(mBackBufferSSR), mClientWidth, mClientHeight, 0, mClientHeight,
                                                    f.flags & CRYCHIC_GBUFFER_F16_MASK, &mSsrParams, &mSsrGlossParams, mCommandList->Stream()));
            frame = bytes(mBackBufferSSR);
        } else if (mScreenSpaceReflections) {   // first: the frame is aligned with the depth plane and the G-buffer, the fog lies over both
            CrychicThrowIfFailed(crychic_ssr(md3dDevice->Ctx(), passCB, f.g0_dev, f.g1_dev, f.g2_dev, f.depth_dev, frame, bytes(mBackBufferSSR), mClientWidth,
                                             mClientHeight, 0, mClientHeight, f.flags & CRYCHIC_GBUFFER_F16_MASK, &mSsrParams, mCommandList->Stream()));
            frame = bytes(mBackBufferSSR);
        }
        if (mFog)
            CrychicThrowIfFailed(crychic_fog(md3dDevice->Ctx(), passCB, f.depth_dev, f.shadow_dev, f.shadowDim, frame, frame,
                                             mClientWidth, mClientHeight, 0, mClientHeight, &mFogParams, mCommandList->Stream()));
        if (mTemporalAA) {                      // blended into the reprojected history while the frame is still aligned with its depth plane
            crychic_taa_params tp = mTaaParams;
            if (mTaaReset) tp.flags |= CRYCHIC_TAA_RESET;
            ID3D12Resource* hin = mTaaHistory[mTaaHistoryIndex].get();
            ID3D12Resource* hout = mTaaHistory[mTaaHistoryIndex ^ 1].get();
            CrychicThrowIfFailed(crychic_taa(md3dDevice->Ctx(), passCB, mTaaViewProj[0], mTaaViewProj[1], f.depth_dev, frame,
                                             mTaaReset ? nullptr : static_cast<const uint16_t*>(hin->Data()), static_cast<uint16_t*>(hout->Data()),
                                             bytes(mBackBufferTAA), mClientWidth, mClientHeight, 0, mClientHeight, &tp, mCommandList->Stream()));
            mTaaHistoryIndex ^= 1;
            mTaaReset = false;
            frame = bytes(mBackBufferTAA);
        }
        uint32_t fw = mClientWidth, fh = mClientHeight;         // the size of `frame`: the display's behind the temporal upsampling
        if (mTemporalUpscale) {                 // at the temporal pass's place; what follows runs at the display size
            crychic_taa_upscale_params tp = mTuParams;
            if (mTuReset) tp.flags |= CRYCHIC_TAA_UPSCALE_RESET;
            ID3D12Resource* hin = mTuHistory[mTuHistoryIndex].get();
            ID3D12Resource* hout = mTuHistory[mTuHistoryIndex ^ 1].get();
            CrychicThrowIfFailed(crychic_taa_upscale(md3dDevice->Ctx(), passCB, mTaaViewProj[0], mTaaViewProj[1], mTaaJitter[0], mTaaJitter[1], f.depth_dev,
                                                     frame, mClientWidth, mClientHeight, mTuReset ? nullptr : static_cast<const uint16_t*>(hin->Data()),
                                                     static_cast<uint16_t*>(hout->Data()), bytes(mBackBufferUpscaled), mTuWidth, mTuHeight, 0, mTuHeight, &tp,
                                                     mCommandList->Stream()));
            mTuHistoryIndex ^= 1;
            mTuReset = false;
            frame = bytes(mBackBufferUpscaled);
            fw = mTuWidth; fh = mTuHeight;
        }
        if (mSharpening) {                      // what the history fetch softened, before the blurs, the bloom and the edge pass work on it
            CrychicThrowIfFailed(crychic_sharpen(md3dDevice->Ctx(), frame, bytes(mBackBufferSharp), fw, fh, 0, fh, &mSharpenParams, mCommandList->Stream()));
            frame = bytes(mBackBufferSharp);
        }
        if (mDepthOfField) {
            CrychicThrowIfFailed(crychic_dof(md3dDevice->Ctx(), passCB, f.depth_dev, frame, bytes(mBackBufferDoF), mClientWidth, mClientHeight, 0,
                                             mClientHeight, &mDofParams, mCommandList->Stream()));
            frame = bytes(mBackBufferDoF);
        }
        if (mMotionBlur) {                      // along the camera's motion since the previous Update
            CrychicThrowIfFailed(crychic_motion_blur(md3dDevice->Ctx(), passCB, mMbViewProj[0], mMbViewProj[1], f.depth_dev, frame, bytes(mBackBufferMB),
                                                     mClientWidth, mClientHeight, &mMbParams, mMbWorkspace->Data(), mMbWorkspace->Bytes(),
                                                     mCommandList->Stream()));
            frame = bytes(mBackBufferMB);
        }
        if (mBloom) {
            CrychicThrowIfFailed(crychic_bloom(md3dDevice->Ctx(), frame, bytes(mBackBufferBloom), fw, fh, &mBloomParams,
                                               mBloomWorkspace->Data(), mBloomWorkspace->Bytes(), mCommandList->Stream()));
            frame = bytes(mBackBufferBloom);
        }
        if (mColourGrade) {                     // the look, in front of the anti-aliasing: its luma test sees graded colours
            CrychicThrowIfFailed(crychic_grade(md3dDevice->Ctx(), frame, bytes(mBackBufferGrade), fw, fh, 0, fh, bytes(mGradeLut), mGradeN,
                                               mCommandList->Stream()));
            frame = bytes(mBackBufferGrade);
        }
        if (mAntiAliasing)
            CrychicThrowIfFailed(crychic_antialias(md3dDevice->Ctx(), frame, bytes(mBackBufferAA), fw, fh, 0, fh,
                                                   &mAAParams, mCommandList->Stream()));
        // :300-305: advance the fence and signal it behind this frame's commands
        mCurrFrameResource->Fence = ++mCurrentFence;
        CrychicHipThrowIfFailed(hipEventRecord(mCurrFrameResource->FenceEvent, mCommandList->Stream()));
    }

    // ---- the passes behind the lighting pass (extensions) -----------------------------------------------------------------------------
    // Ten switches (the temporal upsampling, below, stands at the temporal anti-aliasing's place), all off by default (then nothing changes).  With any of them on, Draw takes a whole frame on one GPU -- SetStrip /
    // JoinNode make it throw, the passes are not sharded -- and issues those that are on behind the lighting pass in the order
    //     lighting -> screen-space reflections (with SetScreenSpaceReflectionGloss: the frame's pyramid and the glossy variant) -> fog (in place) -> temporal anti-aliasing -> sharpening -> depth of field -> motion blur -> bloom -> colour grade -> anti-aliasing.
    // The fog works in place on the frame it is handed: the reflections' buffer if they are on, the back buffer if not.  Every other
    // stage reads the buffer of the nearest stage in front of it that is on and writes one (the back buffer if there is none) and
    // writes a buffer of its own, which exists while the stage is on and which OnResize re-creates; Present writes the last one.
    // CurrentBackBuffer stays the lit frame without them -- fogged unless the reflections took the fog onto their buffer.  A setter's
    // p == nullptr:
    // the pass's default parameters; parameters outside their ranges are refused and leave the switch as it was.

    // ---- anti-aliasing ------------------------------------------------------------------------------------------------------------
    // The deferred path's stand-in for the framework's Set4xMsaaState (Common/d3dApp.cpp:60-70, F2 at :367): MSAA does not compose
    // with a G-buffer, so edges are smoothed by a post-process pass over the finished frame (include/crychic_hip.h
    // crychic_antialias).
    void SetAntiAliasing(bool on, const crychic_aa_params* p = nullptr)
    {
        crychic_aa_params q;
        CrychicThrowIfFailed(crychic_aa_default_params(&q));
        if (p) q = *p;
        if (q.relShift > 31u || q.searchSteps == 0 || q.searchSteps > CRYCHIC_AA_MAX_SEARCH || q.subpix > 256u)
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetAntiAliasing (relShift 0 .. 31, searchSteps 1 .. 16, subpix 0 .. 256)",
                                   __FILE__, __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still write the buffer released below
        mAntiAliasing = on;
        mAAParams = q;
        if (on) mBackBufferAA = FinalPlane();
        else mBackBufferAA.reset();
    }
    bool AntiAliasing() const { return mAntiAliasing; }
    ID3D12Resource* AntiAliasedBackBuffer() { return mBackBufferAA.get(); }

    // ---- fog ------------------------------------------------------------------------------------------------------------------------
    // Volumetric fog with sun shafts through the cascade maps (include/crychic_hip.h crychic_fog), in place on the back buffer.
    void SetFog(bool on, const crychic_fog_params* p = nullptr)
    {
        crychic_fog_params q;
        CrychicThrowIfFailed(crychic_fog_default_params(&q));
        if (p) q = *p;
        if (!(q.density >= 0.0f && q.density <= 16.0f) || !(q.maxDistance > 0.0f && q.maxDistance <= 3.40282347e38f) || q.steps == 0 ||
            q.steps > CRYCHIC_FOG_MAX_STEPS || (q.reserved[0] | q.reserved[1] | q.reserved[2]))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetFog (density 0 .. 16, maxDistance finite and > 0, steps 1 .. 64, reserved 0)",
                                   __FILE__, __LINE__);
        mFog = on;
        mFogParams = q;
    }
    bool Fog() const { return mFog; }

    // ---- screen-space reflections ------------------------------------------------------------------------------------------------------
    // The lit frame's own reflections from the depth plane and the G-buffer (include/crychic_hip.h crychic_ssr), in front of the fog.
    void SetScreenSpaceReflections(bool on, const crychic_ssr_params* p = nullptr)
    {
        crychic_ssr_params q;
        CrychicThrowIfFailed(crychic_ssr_default_params(&q));
        if (p) q = *p;
        const float big = 3.40282347e38f;
        if (!(q.maxDistance > 0.0f && q.maxDistance <= big) || !(q.thickness > 0.0f && q.thickness <= big) || !(q.bias >= 0.0f && q.bias < q.thickness) ||
            !(q.maxRoughness >= 0.0f && q.maxRoughness <= 1.0f) || q.steps == 0 || q.steps > CRYCHIC_SSR_MAX_STEPS || q.edgeFade == 0 || q.edgeFade > 1024u ||
            q.intensity > 256u || q.reserved)
            throw CrychicException(CRYCHIC_E_INVALID_ARG,
                                   "CRYCHIC::SetScreenSpaceReflections (maxDistance and thickness finite and > 0, bias 0 .. thickness, maxRoughness 0 .. 1, "
                                   "steps 1 .. 64, edgeFade 1 .. 1024, intensity 0 .. 256, reserved 0)", __FILE__, __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still write the buffer released below
        mScreenSpaceReflections = on;
        mSsrParams = q;
        if (on) mBackBufferSSR = FramePlane();
        else mBackBufferSSR.reset();
    }
    bool ScreenSpaceReflections() const { return mScreenSpaceReflections; }
    ID3D12Resource* ScreenSpaceReflectionsBackBuffer() { return mBackBufferSSR.get(); }
    // EXPERIMENTAL.  With SetScreenSpaceReflections on too, Draw issues crychic_ssr_pyramid and crychic_ssr_glossy in place of crychic_ssr:
    // the hit colour comes from the level of the lit frame's pyramid that is as wide as the reflection cone at the hit
    // (include/crychic_hip.h).  The default coneScale is 0, the sharp pass: the caller chooses the cone.  On without
    // SetScreenSpaceReflections, Draw throws before it issues anything.
    void SetScreenSpaceReflectionGloss(bool on, const crychic_ssr_gloss_params* p = nullptr)
    {
        crychic_ssr_gloss_params q;
        CrychicThrowIfFailed(crychic_ssr_gloss_default_params(&q));
        if (p) q = *p;
        if (!(q.coneScale >= 0.0f && q.coneScale <= 16.0f) || q.levels == 0 || q.levels > CRYCHIC_SSR_GLOSS_MAX_LEVELS || q.reserved[0] || q.reserved[1])
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetScreenSpaceReflectionGloss (coneScale 0 .. 16, levels 1 .. 8, reserved 0)", __FILE__,
                                   __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still read the pyramid released below
        mSsrGloss = on;
        mSsrGlossParams = q;
        if (on) AllocateSsrPyramid();
        else mSsrPyramid.reset();
    }
    bool ScreenSpaceReflectionGloss() const { return mSsrGloss; }
    ID3D12Resource* ScreenSpaceReflectionPyramid() { return mSsrPyramid.get(); }

    // ---- depth of field ----------------------------------------------------------------------------------------------------------------
    // A thin-lens blur from the depth plane (include/crychic_hip.h crychic_dof).
    void SetDepthOfField(bool on, const crychic_dof_params* p = nullptr)
    {
        crychic_dof_params q;
        CrychicThrowIfFailed(crychic_dof_default_params(&q));
        if (p) q = *p;
        if (!(q.focusDistance > 0.0f && q.focusDistance <= 3.40282347e38f) || !(q.aperture >= 0.0f && q.aperture <= 64.0f) || q.maxRadius == 0 ||
            q.maxRadius > CRYCHIC_DOF_MAX_RADIUS || (q.reserved[0] | q.reserved[1] | q.reserved[2] | q.reserved[3] | q.reserved[4]))
            throw CrychicException(CRYCHIC_E_INVALID_ARG,
                                   "CRYCHIC::SetDepthOfField (focusDistance finite and > 0, aperture 0 .. 64, maxRadius 1 .. 8, reserved 0)", __FILE__,
                                   __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still write the buffer released below
        mDepthOfField = on;
        mDofParams = q;
        if (on) mBackBufferDoF = FramePlane();
        else mBackBufferDoF.reset();
    }
    bool DepthOfField() const { return mDepthOfField; }
    ID3D12Resource* DepthOfFieldBackBuffer() { return mBackBufferDoF.get(); }

    // ---- bloom ----------------------------------------------------------------------------------------------------------------------
    // Highlights over a luma threshold spread through a pyramid and added back (include/crychic_hip.h crychic_bloom), through a
    // workspace this object owns while the pass is on; OnResize re-creates it with the buffer.
    void SetBloom(bool on, const crychic_bloom_params* p = nullptr)
    {
        crychic_bloom_params q;
        CrychicThrowIfFailed(crychic_bloom_default_params(&q));
        if (p) q = *p;
        if (q.threshold > 255u || q.knee == 0u || q.knee > 255u || q.scatter > 256u || q.intensity > 1024u || q.levels == 0u ||
            q.levels > CRYCHIC_BLOOM_MAX_LEVELS || (q.reserved[0] | q.reserved[1] | q.reserved[2]))
            throw CrychicException(CRYCHIC_E_INVALID_ARG,
                                   "CRYCHIC::SetBloom (threshold 0 .. 255, knee 1 .. 255, scatter 0 .. 256, intensity 0 .. 1024, levels 1 .. 8, reserved 0)",
                                   __FILE__, __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still write the buffers released below
        mBloom = on;
        mBloomParams = q;
        if (on) AllocateBloom();
        else { mBackBufferBloom.reset(); mBloomWorkspace.reset(); }
    }
    bool Bloom() const { return mBloom; }
    ID3D12Resource* BloomBackBuffer() { return mBackBufferBloom.get(); }

    // ---- colour grade -------------------------------------------------------------------------------------------------------------------
    // The frame's look through a 3D table, between the bloom and the anti-aliasing (include/crychic_hip.h crychic_grade): the table of
    // an ASC CDL with a saturation, built at CRYCHIC_GRADE_MAX_N (SetColourGrade), a caller's table of N x N x N entries
    // (SetColourGradeLut) or a .cube file (LoadColourGradeLut).  The setter builds or loads the table and uploads it once; Draw issues
    // crychic_grade alone.  nullptr turns the stage off; what is refused leaves it as it was.
    void SetColourGrade(const crychic_grade_params* p)
    {
        if (!p) { SetColourGradeLut(nullptr, 0); return; }
        std::vector<uint8_t> lut((size_t)4 * CRYCHIC_GRADE_MAX_N * CRYCHIC_GRADE_MAX_N * CRYCHIC_GRADE_MAX_N);
        CrychicThrowIfFailed(crychic_grade_build_lut(p, CRYCHIC_GRADE_MAX_N, lut.data(), lut.size()));
        SetColourGradeLut(lut.data(), CRYCHIC_GRADE_MAX_N);
    }
    void SetColourGradeLut(const uint8_t* lut, uint32_t N)
    {
        if (lut && (N < 2u || N > CRYCHIC_GRADE_MAX_N))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetColourGradeLut (N 2 .. 33)", __FILE__, __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still read the table and write the buffer
        mColourGrade = lut != nullptr;
        if (!lut) { mGradeLut.reset(); mBackBufferGrade.reset(); mGradeN = 0; return; }
        const size_t n = (size_t)4 * N * N * N;
        mGradeLut = std::make_unique<ID3D12Resource>(n, ID3D12Resource::DEFAULT_HEAP);
        mGradeLut->Upload(lut, n, mCommandList->Stream());
        mGradeN = N;
        mBackBufferGrade = FinalPlane();
        mCommandList->Flush();                                  // the caller's table may go once this returns
    }
    void LoadColourGradeLut(const char* path)
    {
        std::vector<uint8_t> lut((size_t)4 * CRYCHIC_GRADE_MAX_N * CRYCHIC_GRADE_MAX_N * CRYCHIC_GRADE_MAX_N);
        uint32_t N = 0;
        const int rc = crychic_load_cube_lut(path, lut.data(), lut.size(), &N);
        if (rc < 0) throw CrychicException(rc, "CRYCHIC::LoadColourGradeLut (crychic_load_cube_lut refuses the file)", __FILE__, __LINE__);
        SetColourGradeLut(lut.data(), N);
    }
    bool ColourGrade() const { return mColourGrade; }
    uint32_t ColourGradeSize() const { return mGradeN; }
    ID3D12Resource* ColourGradeBackBuffer() { return mBackBufferGrade.get(); }

    // ---- sharpening --------------------------------------------------------------------------------------------------------------------
    // A contrast-adaptive sharpening of the frame directly behind the temporal stage -- the temporal anti-aliasing or the temporal
    // upsampling, then at the display size -- and in front of the depth of field (include/crychic_hip.h crychic_sharpen); it stands at
    // that place when neither is on.
    void SetSharpening(bool on, const crychic_sharpen_params* p = nullptr)
    {
        crychic_sharpen_params q;
        CrychicThrowIfFailed(crychic_sharpen_default_params(&q));
        if (p) q = *p;
        if (q.strength > CRYCHIC_SHARPEN_MAX_STRENGTH || q.limit > CRYCHIC_SHARPEN_MAX_LIMIT || (q.reserved[0] | q.reserved[1]))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetSharpening (strength 0 .. 256, limit 0 .. 3584, reserved 0)", __FILE__, __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still write the buffer released below
        mSharpening = on;
        mSharpenParams = q;
        if (on) mBackBufferSharp = FinalPlane();
        else mBackBufferSharp.reset();
    }
    bool Sharpening() const { return mSharpening; }
    ID3D12Resource* SharpenedBackBuffer() { return mBackBufferSharp.get(); }

    // ---- temporal anti-aliasing ---------------------------------------------------------------------------------------------------------
    // Jittered frames blended into a reprojected history (include/crychic_hip.h crychic_taa).  On: Update shifts the projection of the
    // main pass and SSAO constants by the frame's sub-pixel offset (crychic_taa_jitter of a running frame index) and keeps the
    // unjittered ViewProj of this frame and of the previous one; Draw issues the pass through two history planes this object owns
    // and swaps.  The first frame after it was turned on, and after OnResize, is a reset frame.  CurrentBackBuffer is then the
    // jittered frame.
    void SetTemporalAA(bool on)
    {
        crychic_taa_params q;
        CrychicThrowIfFailed(crychic_taa_default_params(&q));
        SetTemporalAA(on, q);
    }
    void SetTemporalAA(const crychic_taa_params& p) { SetTemporalAA(true, p); }
    bool TemporalAA() const { return mTemporalAA; }
    ID3D12Resource* TemporalAABackBuffer() { return mBackBufferTAA.get(); }
    ID3D12Resource* TemporalAAHistory() { return mTaaHistory[mTaaHistoryIndex].get(); }     // the history the last Draw wrote
    const float* TemporalAAViewProj(int previous) const { return mTaaViewProj[previous ? 1 : 0]; }   // unjittered, of the last Update
    const float* TemporalAAJitter() const { return mTaaJitter; }                            // the last Update's offset in pixels

    // ---- temporal upsampling ----------------------------------------------------------------------------------------------------------
    // Jittered frames of the client size accumulated into a history of width x height texels (include/crychic_hip.h
    // crychic_taa_upscale), at the temporal anti-aliasing's place in the chain: Update jitters the constants as it does for that pass,
    // Draw issues the pass through two history planes of the display size, and the bloom and the anti-aliasing behind it, their buffers
    // and what Present writes have that size (FinalWidth x FinalHeight).  The first frame after it was turned on, after a change of the
    // display size and after OnResize is a reset frame; the flag is this pass's own.  Draw throws while the temporal anti-aliasing,
    // the depth of field or the motion blur is on as well: the last two read a depth plane of the frame's size.
    void SetTemporalUpscale(uint32_t width, uint32_t height, const crychic_taa_upscale_params* p = nullptr)    // 0 x 0: off
    {
        crychic_taa_upscale_params q;
        CrychicThrowIfFailed(crychic_taa_upscale_default_params(&q));
        if (p) q = *p;
        const bool on = width != 0u || height != 0u;
        if (q.blend == 0u || q.blend > 256u || (q.flags & ~(CRYCHIC_TAA_UPSCALE_RESET | CRYCHIC_TAA_UPSCALE_NO_CLAMP)) ||
            (q.reserved[0] | q.reserved[1] | q.reserved[2] | q.reserved[3] | q.reserved[4] | q.reserved[5]) ||
            (on && (width < (uint32_t)mClientWidth || width > 4u * (uint32_t)mClientWidth || height < (uint32_t)mClientHeight || height > 4u * (uint32_t)mClientHeight)))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetTemporalUpscale (each side 1 .. 4 times the client's, blend 1 .. 256, flags RESET | NO_CLAMP, reserved 0)",
                                   __FILE__, __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still write the buffers released below
        const bool was = mTemporalUpscale, resized = width != mTuWidth || height != mTuHeight;
        mTemporalUpscale = on;
        mTuParams = q;
        mTuWidth = width; mTuHeight = height;
        if (on && (!was || resized)) AllocateTemporalUpscale();
        if (on && !was) mTaaFrameIndex = 0;
        if (!on) { mBackBufferUpscaled.reset(); mTuHistory[0].reset(); mTuHistory[1].reset(); }
        if (was != on || resized) {                             // the stages behind it change their size with it
            if (mAntiAliasing) mBackBufferAA = FinalPlane();
            if (mBloom) AllocateBloom();
            if (mColourGrade) mBackBufferGrade = FinalPlane();
            if (mSharpening) mBackBufferSharp = FinalPlane();
        }
    }
    bool TemporalUpscale() const { return mTemporalUpscale; }
    ID3D12Resource* TemporalUpscaleBackBuffer() { return mBackBufferUpscaled.get(); }
    ID3D12Resource* TemporalUpscaleHistory() { return mTuHistory[mTuHistoryIndex].get(); }  // the history the last Draw wrote
    uint32_t FinalWidth() const { return mTemporalUpscale ? mTuWidth : (uint32_t)mClientWidth; }      // of FinalFrame
    uint32_t FinalHeight() const { return mTemporalUpscale ? mTuHeight : (uint32_t)mClientHeight; }

    // ---- motion blur ------------------------------------------------------------------------------------------------------------------
    // Camera motion turned into blur (include/crychic_hip.h crychic_motion_blur).  On: Update keeps the unjittered ViewProj of this
    // frame and of the previous one (the first frame after it was turned on, and after OnResize, has no previous one: a still
    // camera); Draw issues the pass through a workspace this object owns while the pass is on.
    void SetMotionBlur(bool on, const crychic_motion_blur_params* p = nullptr)
    {
        crychic_motion_blur_params q;
        CrychicThrowIfFailed(crychic_motion_blur_default_params(&q));
        if (p) q = *p;
        if (q.shutter > 256u || q.samples < 2u || q.samples > 32u || (q.samples & (q.samples - 1u)) || q.maxRadius == 0u || q.maxRadius > 32u || q.flags ||
            (q.reserved[0] | q.reserved[1] | q.reserved[2] | q.reserved[3]))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetMotionBlur (shutter 0 .. 256, samples 2, 4, 8, 16 or 32, maxRadius 1 .. 32, flags 0, reserved 0)",
                                   __FILE__, __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still write the buffers released below
        const bool was = mMotionBlur;
        mMotionBlur = on;
        mMbParams = q;
        if (on && !was) AllocateMotionBlur();
        if (!on) { mBackBufferMB.reset(); mMbWorkspace.reset(); }
    }
    bool MotionBlur() const { return mMotionBlur; }
    ID3D12Resource* MotionBlurBackBuffer() { return mBackBufferMB.get(); }
    ID3D12Resource* MotionBlurWorkspace() { return mMbWorkspace.get(); }
    const float* MotionBlurViewProj(int previous) const { return mMbViewProj[previous ? 1 : 0]; }   // unjittered, of the last Update

    // ---- deferred decals (extension) ------------------------------------------------------------------------------------------------
    // Oriented boxes that blend textures into the G-buffer between the producer passes and the lighting pass (include/crychic_hip.h
    // crychic_apply_decals; crychic_decal_from_box fills a decal from a matrix).  SetDecals uploads the n <= CRYCHIC_MAX_DECALS decals to
    // a device buffer this object owns and copies the table of nTex <= CRYCHIC_DECAL_MAX_TEXTURES textures (device pointers the caller
    // keeps alive).  While decals are set and mRunProducerPasses is on, Draw issues the pass behind the camera producer passes, for the
    // rows it draws: it is valid with SetStrip / JoinNode, each GPU decaling its own strip.  With mRunProducerPasses off Draw leaves the
    // caller's planes alone (a second application would stack).  The probe of CaptureEnvironment is an object of its own and has no
    // decals: captures do not show them.  The SSAO pass's view-normal map is not touched.  With none set (the default) Draw issues
    // exactly the calls it issues without this extension.  Waits for the frames in flight first, which may still read the buffer.
    void SetDecals(const crychic_decal* decals, uint32_t n, const crychic_texture* textures, uint32_t nTex)
    {
        if (n > CRYCHIC_MAX_DECALS || nTex > CRYCHIC_DECAL_MAX_TEXTURES || (n && !decals) || (nTex && !textures))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetDecals (at most 64 decals and 16 textures, non-null when non-empty)", __FILE__,
                                   __LINE__);
        mCommandList->Flush();
        mDecals.reset();
        mDecalCount = 0;
        mDecalTextures.assign(textures, textures + nTex);
        if (n == 0) return;
        mDecals = std::make_unique<ID3D12Resource>((size_t)n * sizeof(crychic_decal), ID3D12Resource::DEFAULT_HEAP);
        mDecals->Upload(decals, (size_t)n * sizeof(crychic_decal), mCommandList->Stream());
        mDecalCount = n;
        mCommandList->Flush();                  // the caller's array may go once this returns
    }
    void ClearDecals() { SetDecals(nullptr, 0, nullptr, 0); }
    uint32_t DecalCount() const { return mDecalCount; }

    // ---- local lights (extension: the reference's point and spot branches, PBR.hlsl:109-147, are dead code) -------------------
    // Uploads both lists to device buffers this object owns (at most 1024 each); Draw lights them after the directional lights,
    // point lights first, on the single-GPU and the shared path alike (include/crychic_hip.h crychic_deferred_light_spots).
    // nullptr / 0 for a list removes it; both empty = the reference configuration.  Waits for the frames in flight first, which
    // may still read the previous buffers.
    void SetLocalLights(const Light* points, uint32_t nPoints, const Light* spots, uint32_t nSpots)
    {
        static_assert(sizeof(Light) == sizeof(crychic_light), "Light is crychic_light");
        if (nPoints > 1024u || nSpots > 1024u || (nPoints && !points) || (nSpots && !spots))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetLocalLights (at most 1024 lights per list, non-null when non-empty)",
                                   __FILE__, __LINE__);
        mCommandList->Flush();
        auto upload = [&](const Light* src, uint32_t n, std::unique_ptr<ID3D12Resource>& dst, uint32_t& count) {
            dst.reset();
            count = 0;
            if (n == 0) return;
            dst = std::make_unique<ID3D12Resource>((size_t)n * sizeof(Light), ID3D12Resource::DEFAULT_HEAP);
            dst->Upload(src, (size_t)n * sizeof(Light), mCommandList->Stream());
            count = n;
        };
        upload(points, nPoints, mPointLights, mNumPointLights);
        upload(spots, nSpots, mSpotLights, mNumSpotLights);
        mSpotHost.assign(spots, spots + nSpots);    // the shadow transforms are built from these
        mPointHost.assign(points, points + nPoints);
        if (mSpotShadowCount > nSpots) SetSpotShadows(0, 0, 0.0f, 0.0f);
        if (mPointShadowCount > nPoints) SetPointShadows(0, 0, 0.0f);
        UpdatePointShadowTransforms();          // the faces follow the lights that keep their shadows
        mCommandList->Flush();                  // the caller's arrays may go once this returns
    }

    // ---- shadowed spot lights (extension: the reference reserves gShadowMap[4..11] / gShadowTransforms[4..11] and leaves them
    // empty, Common.hlsl:46,91) -----------------------------------------------------------------------------------------------
    // The first `count` (<= 8, at most the spot lights of SetLocalLights) spot lights cast shadows: each gets a dim x dim D24 map that
    // DrawSceneToShadowMap renders after the four cascades (perspective, fovY, zNear .. FalloffEnd; crychic_update_spot_shadow_transform)
    // and ShadowTransforms[4 + k]; Draw hands them to the lighting pass (include/crychic_hip.h crychic_deferred_light_spots_shadowed).
    // count 0 removes the shadows.  Waits for the frames in flight first, which may still read the previous maps.
    void SetSpotShadows(uint32_t count, uint32_t dim, float fovY, float zNear)
    {
        mCommandList->Flush();
        mSpotShadowMaps.clear();
        mSpotShadowCount = 0;
        if (count == 0) return;
        if (count > CRYCHIC_MAX_SPOT_SHADOWS || count > mNumSpotLights || dim < 2 || dim > CRYCHIC_MAX_SPOT_SHADOW_DIM)
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetSpotShadows (count 1 .. 8 and at most the spot lights, dim 2 .. 16384)",
                                   __FILE__, __LINE__);
        float v[16], p[16], t[16];
        for (uint32_t k = 0; k < count; ++k)       // fovY / zNear against every light's range, before anything changes
            CrychicThrowIfFailed(crychic_update_spot_shadow_transform(reinterpret_cast<const crychic_light*>(&mSpotHost[k]), fovY, zNear, v, p, t));
        for (uint32_t k = 0; k < count; ++k)
            mSpotShadowMaps.push_back(std::make_unique<ID3D12Resource>((size_t)dim * dim * 4u, ID3D12Resource::DEFAULT_HEAP));
        mSpotShadowCount = count;
        mSpotShadowDim = dim;
        mSpotShadowFovY = fovY;
        mSpotShadowZNear = zNear;
        UpdateSpotShadowTransforms();
    }
    ID3D12Resource* SpotShadowMap(uint32_t k) { return k < mSpotShadowCount ? mSpotShadowMaps[k].get() : nullptr; }

    // ---- shadowed point lights (extension: cube shadows, include/crychic_hip.h crychic_deferred_light_point_shadows) -------------
    // The first `count` (<= 4, at most the point lights of SetLocalLights) point lights cast shadows: each gets six dim x dim D24 faces
    // (+X, -X, +Y, -Y, +Z, -Z back to back) that DrawSceneToShadowMap renders after the spot lights' maps (widened 90-degree faces,
    // zNear .. FalloffEnd; crychic_update_point_shadow_transforms); Draw takes the _point_shadows entries.  count 0 removes the shadows,
    // and SetLocalLights drops them when fewer point lights remain.  Waits for the frames in flight first, which may still read the faces.
    void SetPointShadows(uint32_t count, uint32_t dim, float zNear)
    {
        mCommandList->Flush();
        mPointShadowMaps.clear();
        mPointShadowCount = 0;
        if (count == 0) return;
        if (count > CRYCHIC_MAX_POINT_SHADOWS || count > mNumPointLights || dim < CRYCHIC_MIN_POINT_SHADOW_DIM || dim > CRYCHIC_MAX_SPOT_SHADOW_DIM)
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetPointShadows (count 1 .. 4 and at most the point lights, dim 16 .. 16384)",
                                   __FILE__, __LINE__);
        float v[6][16], p[16], t[16];
        for (uint32_t k = 0; k < count; ++k)       // zNear against every light's range, before anything changes
            CrychicThrowIfFailed(crychic_update_point_shadow_transforms(reinterpret_cast<const crychic_light*>(&mPointHost[k]), dim, zNear, v, p, t));
        for (uint32_t k = 0; k < count; ++k)
            mPointShadowMaps.push_back(std::make_unique<ID3D12Resource>((size_t)6 * dim * dim * 4u, ID3D12Resource::DEFAULT_HEAP));
        mPointShadowCount = count;
        mPointShadowDim = dim;
        mPointShadowZNear = zNear;
        UpdatePointShadowTransforms();
    }
    // The six faces of point light k, back to back (nullptr when it has none).
    ID3D12Resource* PointShadowMap(uint32_t k) { return k < mPointShadowCount ? mPointShadowMaps[k].get() : nullptr; }

    // ---- environment capture (extension: include/crychic_hip.h "environment capture") -------------------------------------------
    // Renders the built-in scene this object draws into a cube map at (x, y, z) and binds it: face f of level 0 is the frame Draw
    // produces at dim x dim for face camera f (crychic_cube_capture_cameras; zNear 0.5, the main lens's far plane) with the sky on,
    // written in place by a dim x dim probe this object keeps (its own planes and cascades of shadowDim, its own copy of the built-in
    // scene); the local lights, their shadow maps (rendered here first when there are any: call Update before), the cube map, the
    // G-buffer formats, the textures, blurCount and the timer are this object's, read in place.  crychic_generate_cube_mips then
    // builds `levels` levels (0 = down to 1 x 1) and SetCubeMap binds the chain.  The cube map bound before is the source -- a capture
    // never reflects itself, two captures in a row give one bounce -- and becomes the next capture's destination when its size fits,
    // so a per-frame re-capture allocates nothing.  An object whose planes the caller fills (mRunProducerPasses == false) has no scene
    // to capture and is refused.  With SetGlossyReflections(true) the faces and their box chain go to a scratch chain this object
    // keeps, and the chain bound is crychic_prefilter_cube_chain's of it.  With SetEnvironmentAmbient(true) the chain is allocated with
    // its environment tail (crychic_cube_chain_sh_bytes) and level 0 of the box chain is projected into it (crychic_project_cube_sh);
    // a chain of more than one level then needs SetGlossyReflections(true) (the derivative-LOD chain has no such kernels).  With
    // SetEnvironmentSpecular(true) -- which needs SetGlossyReflections(true) and more than one level -- the chain is allocated with the
    // environment tail and the environment BRDF table (crychic_cube_chain_env_bytes) and the table is built behind the tail
    // (crychic_build_env_brdf).  The capture position is remembered; with SetReflectionProbeBox's box set and glossy reflections on over
    // more than one level the chain is allocated with its environment tail at least, and the probe volume -- (x, y, z) and the box --
    // is written into the tail of the chain that is bound (crychic_set_cube_probe_volume; a box that does not hold the position
    // strictly inside is refused before anything is rendered).
    void CaptureEnvironment(float x, float y, float z, UINT dim, UINT levels = 0, UINT shadowDim = 1024)
    {
        uint32_t full = 1;
        for (UINT m = dim; m > 1u; m >>= 1) ++full;
        if (full > 15u) full = 15u;
        if (levels == 0) levels = full;
        const bool localShadows = mSpotShadowCount > 0 || mPointShadowCount > 0;
        if (!mCubeMap || !mRunProducerPasses || (localShadows && !mCurrFrameResource) || dim == 0 || (dim & 1u) || dim > 8192u ||
            levels > full || shadowDim < 2u)
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::CaptureEnvironment (a cube map bound as the source; the producer passes on; "
                                   "Update before it with shadowed local lights; dim even, 2 .. 8192; at most floor(log2 dim) + 1 levels)",
                                   __FILE__, __LINE__);
        if (mEnvironmentAmbient && levels > 1u && !mGlossyReflections)
            throw CrychicException(CRYCHIC_E_UNSUPPORTED, "CRYCHIC::CaptureEnvironment (environment ambient with a chain needs glossy reflections)",
                                   __FILE__, __LINE__);
        if (mEnvironmentSpecular && (levels < 2u || !mGlossyReflections))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::CaptureEnvironment (environment specular needs glossy reflections and a chain)",
                                   __FILE__, __LINE__);
        if (localShadows) {                     // the probe reads this object's local-light shadow maps: as Draw would render them now
            auto items = DrawItems(mRitemLayer[(int)RenderLayer::OpaqueShadow]);
            if (mSpotShadowCount > 0) DrawSpotShadowMaps(items);
            if (mPointShadowCount > 0) DrawPointShadowMaps(items);
        }
        mCommandList->Flush();                  // what the probe's stream reads is complete
        if (!mProbe || mProbe->mClientWidth != dim || mProbe->mShadowMapSize != shadowDim) {
            mProbe.reset();
            mProbe = std::make_unique<CRYCHIC>(mDeviceOrdinal, dim, dim);
            mProbe->mShadowMapSize = shadowDim;
            mProbe->Initialize();
            mProbe->mSsao->CopyNoiseFrom(*mSsao, mProbe->mCommandList.get());      // the SSAO noise is view-independent: this object's
            mProbe->mOwner = this;
        }
        CRYCHIC& p = *mProbe;
        p.mBlurCount = mBlurCount; p.mNumDirLights = mNumDirLights; p.mPcfLiteral = mPcfLiteral; p.mSkyEnabled = true;
        p.mFrustumCullingEnabled = mFrustumCullingEnabled; p.mFuseCameraPasses = mFuseCameraPasses;
        for (int i = 0; i < 3; ++i) p.mBaseLightDirections[i] = mBaseLightDirections[i];
        p.mLightRotationAngle = mLightRotationAngle;
        if (p.mDeferred->FormatFlags() != mDeferred->FormatFlags()) p.SetGBufferFormat(mDeferred->Format(0), mDeferred->Format(1), mDeferred->Format(2));
        p.mTextures = mTextures;                // the device copies stay this object's (mTexturePlanes)
        const size_t faceBytes = (size_t)dim * dim * 4u, chainBytes = crychic_cube_chain_bytes(dim, levels);
        const bool withProbe = mProbeBoxSet && mGlossyReflections && levels > 1u;                                  // the probe volume lives in the tail
        const size_t boundBytes = mEnvironmentSpecular ? crychic_cube_chain_env_bytes(dim, levels)                  // with the tail and the table
                                : (mEnvironmentAmbient || withProbe) ? crychic_cube_chain_sh_bytes(dim, levels) : chainBytes;     // with the environment tail
        std::unique_ptr<ID3D12Resource> chain = std::move(mSpareCubeMap);          // the cube map the last capture replaced
        if (!chain || chain->Bytes() != boundBytes) chain = std::make_unique<ID3D12Resource>(boundBytes, ID3D12Resource::DEFAULT_HEAP);
        if (mGlossyReflections && (!mCaptureBoxChain || mCaptureBoxChain->Bytes() != chainBytes))
            mCaptureBoxChain = std::make_unique<ID3D12Resource>(chainBytes, ID3D12Resource::DEFAULT_HEAP);
        ID3D12Resource* box = mGlossyReflections ? mCaptureBoxChain.get() : chain.get();         // where the faces are rendered
        const float pos[3] = { x, y, z };
        if (withProbe)                          // the prefilter and the projection leave tail bytes [368, 416) alone
            CrychicThrowIfFailed(crychic_set_cube_probe_volume(md3dDevice->Ctx(), static_cast<uint8_t*>(chain->Data()) + crychic_cube_sh_offset(dim, levels),
                                                               pos, mProbeBoxMin, mProbeBoxMax, mCommandList->Stream()));
        crychic_camera cams[6];
        CrychicThrowIfFailed(crychic_cube_capture_cameras(pos, 0.5f, mCamera.GetFarZ(), cams));
        for (int f = 0; f < 6; ++f) {
            const crychic_camera& c = cams[f];
            p.mCamera.SetPosition(c.pos[0], c.pos[1], c.pos[2]);
            p.mCamera.LookTo(c.look[0], c.look[1], c.look[2], c.up[0], c.up[1], c.up[2]);
            p.mCamera.SetLens(c.fovY, c.aspect, c.nearZ, c.farZ);
            p.mRenderTarget = static_cast<uint8_t*>(box->Data()) + (size_t)f * faceBytes;
            p.Update(mLastTimer);
            p.Draw(mLastTimer);
        }
        p.mCommandList->Flush();
        p.mRenderTarget = nullptr;
        CrychicThrowIfFailed(crychic_generate_cube_mips(md3dDevice->Ctx(), static_cast<uint8_t*>(box->Data()), dim, levels, mCommandList->Stream()));
        if (mEnvironmentAmbient)                // the box chain's level 0 (the prefiltered chain's level 0 is its copy) into the bound chain's tail
            CrychicThrowIfFailed(crychic_project_cube_sh(md3dDevice->Ctx(), static_cast<const uint8_t*>(box->Data()), dim,
                                                         static_cast<uint8_t*>(chain->Data()) + crychic_cube_sh_offset(dim, levels),
                                                         mCommandList->Stream()));
        if (mEnvironmentSpecular)               // the table depends on nothing but its definition: built where the bound chain keeps it
            CrychicThrowIfFailed(crychic_build_env_brdf(md3dDevice->Ctx(), static_cast<uint8_t*>(chain->Data()) + crychic_cube_env_brdf_offset(dim, levels),
                                                        mCommandList->Stream()));
        if (mGlossyReflections)
            CrychicThrowIfFailed(crychic_prefilter_cube_chain(md3dDevice->Ctx(), static_cast<const uint8_t*>(box->Data()),
                                                              static_cast<uint8_t*>(chain->Data()), dim, levels, mCommandList->Stream()));
        mCommandList->Flush();                  // frames in flight may still read the source, which the next capture overwrites
        mSpareCubeMap = std::move(mCubeMap);
        SetCubeMap(std::move(chain), dim, levels, mEnvironmentAmbient, mEnvironmentSpecular);
        mCubeMapHasProbe = withProbe;
        mCapturePos[0] = x; mCapturePos[1] = y; mCapturePos[2] = z; mHaveCapturePos = true;
    }

    // ---- one frame on several GPUs (no counterpart in the single-GPU reference) ----------------------------------
    // Rows [row0, row0 + rows) are this GPU's share of the hot path (row0 even).  An empty share is refused: a rank without rows
    // would have nothing to contribute to the gather (and "0 rows" must never come to mean "the whole frame").
    void SetStrip(UINT row0, UINT rows)
    {
        if (rows == 0 || row0 >= mClientHeight || rows > mClientHeight - row0)
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetStrip (empty strip or rows outside the frame)", __FILE__, __LINE__);
        mStripRow0 = row0; mStripRows = rows; mWholeFrame = false;
    }
    void SetWholeFrame() { mStripRow0 = 0; mStripRows = 0; mWholeFrame = true; }
    // One process per GPU: `id` is the rendezvous id rank 0 obtained from crychic_comm_unique_id and handed to its peers.
    // Takes the crychic_strip_rows plan unless `bounds` (nranks x {row0, rows}) gives another tiling.
    void JoinNode(int nranks, int rank, const uint8_t id[CRYCHIC_COMM_ID_BYTES], const std::vector<uint32_t>& bounds = {})
    {
        LeaveNode();
        CrychicThrowIfFailed(crychic_comm_create(md3dDevice->Ctx(), nranks, rank, id, &mComm));
        mStripBounds = bounds;
        uint32_t r0 = 0, rn = 0;
        if (bounds.empty()) CrychicThrowIfFailed(crychic_strip_rows(mClientHeight, nranks, rank, &r0, &rn));
        else { r0 = bounds.at(2 * (size_t)rank); rn = bounds.at(2 * (size_t)rank + 1); }
        SetStrip(r0, rn);
    }
    // 1 (default): the strip, then one exchange.  n > 1: the shared hot path's overlapped exchange in n parts.
    void SetExchangeParts(UINT n)
    {
        if (n == 0 || n > CRYCHIC_MAX_EXCHANGE_PARTS) throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetExchangeParts", __FILE__, __LINE__);
        mExchangeParts = n;
    }
    void LeaveNode()
    {
        if (mComm) { mCommandList->Flush(); crychic_comm_destroy(mComm); mComm = nullptr; }
        mStripBounds.clear();
        SetWholeFrame();
    }

    // mSwapChain->Present (CRYCHIC.cpp:294-297) for a headless build: read the finished frame back -- the buffer of the last stage
    // that is on, the back buffer if none is -- and write it as PPM.
    void Present(const std::string& path)
    {
        std::vector<uint8_t> host((size_t)FinalWidth() * FinalHeight() * 4);
        FinalFrame()->Download(host.data(), host.size(), mCommandList->Stream());
        mCommandList->Flush();
        CrychicThrowIfFailed(crychic_save_ppm(path.c_str(), host.data(), FinalWidth(), FinalHeight()));
    }

    // ---- planes the producer passes would fill (row f1) + the result ----
    ID3D12Resource* DepthStencilBuffer() { return mDepthStencilBuffer.get(); }
    ID3D12Resource* CurrentBackBuffer() { return mBackBuffer.get(); }
    // `levels` > 1: the resource holds the mip chain in crychic_load_dds_cube_rgba8_mips' layout (the reference binds every level,
    // CRYCHIC.cpp:1148-1151) and Draw announces it with CRYCHIC_LIGHT_CUBE_LEVELS
    ID3D12Resource* CubeMap() { return mCubeMap.get(); }
    UINT CubeMapSize() const { return mCubeMapSize; }
    UINT CubeMapLevels() const { return mCubeMapLevels; }
    // hasTail: the resource holds crychic_cube_chain_sh_bytes(dim, levels) bytes, the cube map and behind it the environment tail
    // crychic_project_cube_sh filled; Draw then announces CRYCHIC_LIGHT_AMBIENT_SH.
    // hasTable: the resource holds crychic_cube_chain_env_bytes(dim, levels) bytes, and behind the environment tail (filled or not) the
    // table crychic_build_env_brdf made; Draw then announces CRYCHIC_LIGHT_ENV_BRDF whenever it announces CRYCHIC_LIGHT_CUBE_GLOSS.
    void SetCubeMap(std::unique_ptr<ID3D12Resource> cube, UINT dim, UINT levels = 1, bool hasTail = false, bool hasTable = false)
    {
        mCubeMap = std::move(cube); mCubeMapSize = dim; mCubeMapLevels = levels ? levels : 1; mCubeMapHasTail = hasTail;
        mCubeMapHasTable = hasTable;
        mCubeMapHasProbe = false;               // CaptureEnvironment and SetReflectionProbeBox write the volume and say so
        mHaveCapturePos = false;
        mSkyOf = nullptr;                       // SetProceduralSky: whatever is bound now is not (yet) the sky Draw rendered
    }
    bool CubeMapHasTail() const { return mCubeMapHasTail; }
    bool CubeMapHasTable() const { return mCubeMapHasTable; }
    // Split-sum specular from the environment (extension: include/crychic_hip.h CRYCHIC_LIGHT_ENV_BRDF): while on, CaptureEnvironment
    // (with glossy reflections on) allocates the chain with the environment BRDF table behind its environment tail and builds it;
    // Draw -- this object's and its probe's -- weighs the glossy reflection of a bound chain that has a table by the split sum's
    // second factor instead of shininess and the mirror direction's Fresnel term.
    void SetEnvironmentSpecular(bool on) { mEnvironmentSpecular = on; }
    bool EnvironmentSpecular() const { return mEnvironmentSpecular; }
    // Ambient light from the environment (extension: include/crychic_hip.h CRYCHIC_LIGHT_AMBIENT_SH): while on, CaptureEnvironment
    // allocates the chain with its environment tail and projects the captured level 0 onto the nine SH9 irradiance coefficients;
    // Draw -- this object's and its probe's -- takes the ambient colour from the tail of a bound cube map that has one.
    void SetEnvironmentAmbient(bool on) { mEnvironmentAmbient = on; }
    bool EnvironmentAmbient() const { return mEnvironmentAmbient; }
    // Parallax-corrected reflections (extension: include/crychic_hip.h CRYCHIC_LIGHT_CUBE_PARALLAX): the axis-aligned proxy box of the
    // captured surroundings.  While a box is set, CaptureEnvironment (with glossy reflections on) writes the probe volume -- its own
    // position and the box -- into the environment tail of the chain it binds, and Draw -- this object's and its probe's -- looks a
    // glossy chain that has the volume up along the box-projected direction.  Set after a capture whose chain has a tail, the volume
    // is written at once with the remembered capture position.  ClearReflectionProbeBox clears the flag: the distant lookup again.
    void SetReflectionProbeBox(const float boxMin[3], const float boxMax[3])
    {
        for (int k = 0; k < 3; ++k) { mProbeBoxMin[k] = boxMin[k]; mProbeBoxMax[k] = boxMax[k]; }
        mProbeBoxSet = true;
        if (mHaveCapturePos && mCubeMap && mCubeMapLevels > 1 && mCubeMap->Bytes() >= crychic_cube_chain_sh_bytes(mCubeMapSize, mCubeMapLevels)) {
            mCommandList->Flush();              // frames in flight read the volume that is there
            CrychicThrowIfFailed(crychic_set_cube_probe_volume(md3dDevice->Ctx(), static_cast<uint8_t*>(mCubeMap->Data()) + crychic_cube_sh_offset(mCubeMapSize, mCubeMapLevels),
                                                               mCapturePos, mProbeBoxMin, mProbeBoxMax, mCommandList->Stream()));
            mCubeMapHasProbe = true;
        }
    }
    void ClearReflectionProbeBox() { mProbeBoxSet = false; }
    bool ReflectionProbeBox() const { return mProbeBoxSet; }
    bool CubeMapHasProbe() const { return mCubeMapHasProbe; }
    // Glossy reflections (extension: include/crychic_hip.h CRYCHIC_LIGHT_CUBE_GLOSS): while on, CaptureEnvironment binds the captured
    // chain prefiltered by roughness, and Draw -- this object's and its probe's -- looks a bound chain (more than one level) up at the
    // level of the pixel's roughness.  The caller turns it on for a chain that is prefiltered: a capture made while it is on, or one
    // it ran crychic_prefilter_cube_chain over.
    void SetGlossyReflections(bool on) { mGlossyReflections = on; }
    bool GlossyReflections() const { return mGlossyReflections; }

    // Procedural sky (extension: include/crychic_hip.h "procedural sky"; no counterpart: the reference's sky is
    // a file).  Renders the single-scattering atmosphere of `params` (nullptr = the defaults) into level 0 of a chain of `levels`
    // levels (0 = the full chain) of `dim`-texel faces (0 = the bound cube map's size, 256 if none is bound) and binds it, shaped like
    // CaptureEnvironment: the mip chain, and with SetEnvironmentAmbient / SetEnvironmentSpecular / SetGlossyReflections on the SH
    // projection of level 0, the environment BRDF table and the prefilter, in that order, refused in the same combinations.  The cube
    // map bound before becomes the next call's destination when its size fits, so a per-frame re-render allocates nothing.
    void RenderSky(const crychic_sky_params* params = nullptr, UINT dim = 0, UINT levels = 0)
    {
        if (dim == 0) dim = mCubeMap ? mCubeMapSize : 256u;
        uint32_t full = 1;
        for (UINT m = dim; m > 1u; m >>= 1) ++full;
        if (full > 15u) full = 15u;
        if (levels == 0) levels = full;
        if (dim < 2u || dim > 8192u || levels > full)
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::RenderSky (dim 2 .. 8192; at most floor(log2 dim) + 1 levels)", __FILE__, __LINE__);
        if (mEnvironmentAmbient && levels > 1u && !mGlossyReflections)
            throw CrychicException(CRYCHIC_E_UNSUPPORTED, "CRYCHIC::RenderSky (environment ambient with a chain needs glossy reflections)", __FILE__, __LINE__);
        if (mEnvironmentSpecular && (levels < 2u || !mGlossyReflections))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::RenderSky (environment specular needs glossy reflections and a chain)", __FILE__, __LINE__);
        const bool gloss = mGlossyReflections && levels > 1u;
        const size_t chainBytes = crychic_cube_chain_bytes(dim, levels);
        const size_t boundBytes = mEnvironmentSpecular ? crychic_cube_chain_env_bytes(dim, levels)
                                : mEnvironmentAmbient ? crychic_cube_chain_sh_bytes(dim, levels) : chainBytes;
        std::unique_ptr<ID3D12Resource> chain = std::move(mSpareCubeMap);
        if (!chain || chain->Bytes() != boundBytes) chain = std::make_unique<ID3D12Resource>(boundBytes, ID3D12Resource::DEFAULT_HEAP);
        if (gloss && (!mCaptureBoxChain || mCaptureBoxChain->Bytes() != chainBytes))
            mCaptureBoxChain = std::make_unique<ID3D12Resource>(chainBytes, ID3D12Resource::DEFAULT_HEAP);
        ID3D12Resource* box = gloss ? mCaptureBoxChain.get() : chain.get();
        crychic_ctx* ctx = md3dDevice->Ctx();
        CrychicThrowIfFailed(crychic_render_sky(ctx, static_cast<uint8_t*>(box->Data()), dim, 0, 6, params, mCommandList->Stream()));
        ++mSkyRenders;
        CrychicThrowIfFailed(crychic_generate_cube_mips(ctx, static_cast<uint8_t*>(box->Data()), dim, levels, mCommandList->Stream()));
        if (mEnvironmentAmbient)
            CrychicThrowIfFailed(crychic_project_cube_sh(ctx, static_cast<const uint8_t*>(box->Data()), dim,
                                                         static_cast<uint8_t*>(chain->Data()) + crychic_cube_sh_offset(dim, levels), mCommandList->Stream()));
        if (mEnvironmentSpecular)
            CrychicThrowIfFailed(crychic_build_env_brdf(ctx, static_cast<uint8_t*>(chain->Data()) + crychic_cube_env_brdf_offset(dim, levels),
                                                        mCommandList->Stream()));
        if (gloss)
            CrychicThrowIfFailed(crychic_prefilter_cube_chain(ctx, static_cast<const uint8_t*>(box->Data()), static_cast<uint8_t*>(chain->Data()), dim,
                                                              levels, mCommandList->Stream()));
        mCommandList->Flush();                  // frames in flight may still read the cube map bound so far, the next call's destination
        mSpareCubeMap = std::move(mCubeMap);
        SetCubeMap(std::move(chain), dim, levels, mEnvironmentAmbient, mEnvironmentSpecular);
    }
    // While `follow` is on, Draw takes the sky's sunDir from -mMainPassCB.Lights[0].Direction in front of the lighting frame and, when
    // the direction or the parameters are not those of the sky it rendered last (or another cube map was bound since), calls
    // RenderSky(params with that sun, the bound size and levels).  Off, Draw issues exactly the calls it issues without it.
    void SetProceduralSky(bool follow, const crychic_sky_params* params = nullptr)
    {
        crychic_sky_params p;
        CrychicThrowIfFailed(crychic_sky_default_params(&p));
        if (params) p = *params;
        float rgb[3];
        CrychicThrowIfFailed(crychic_sky_sun_colour(&p, rgb));      // a parameter outside its range is refused here and leaves the switch as it was
        mSkyParams = p; mFollowSun = follow; mSkyOf = nullptr;
    }
    bool ProceduralSky() const { return mFollowSun; }
    // The angle about +y the next Update turns the three directional lights by.  The reference's own rate is zero (:152), so its
    // lights stand still; an application that moves its sun sets the angle here, and the shadows, the lighting and -- under
    // SetProceduralSky -- the sky follow from the same pass constants.
    void SetLightRotationAngle(float radians) { mLightRotationAngle = radians; }
    float LightRotationAngle() const { return mLightRotationAngle; }
    // Draw's part of SetProceduralSky
    void FollowSun()
    {
        const auto& d = mMainPassCB.Lights[0].Direction;
        const float sun[3] = { -d.x, -d.y, -d.z };
        if (mSkyOf && mSkyOf == mCubeMap.get() && std::memcmp(sun, mSkyParams.sunDir, sizeof sun) == 0) return;
        std::memcpy(mSkyParams.sunDir, sun, sizeof sun);
        RenderSky(&mSkyParams, mCubeMap ? mCubeMapSize : 0u, mCubeMap ? mCubeMapLevels : 1u);
        mSkyOf = mCubeMap.get();
    }
    UINT SkyRenders() const { return mSkyRenders; }     // launches of crychic_render_sky this object has issued

    // CRYCHIC::LoadTextures (CRYCHIC.cpp:939-973): the six material textures in heap order (= gTextureMaps indices, :954-959) with the
    // mip chains their files store, and the sky cube map, from `dir` (the reference opens "Textures/...").  The DDS decoding that
    // CreateDDSTextureFromFile12 + the texture units do is done on the host (crychic_load_dds_*); a missing cube file keeps the
    // cube map set through SetCubeMap (snowcube1024.dds is not part of the reference checkout).
    void LoadTextures(const std::string& dir, bool requireCubeMap = false)
    {
        static const char* const files[6] = { "bricks2.dds", "bricks2_nmap.dds", "tile.dds", "tile_nmap.dds", "white1x1.dds", "default_nmap.dds" };
        hipStream_t s = mCommandList->Stream();
        std::vector<crychic_texture> tex;
        std::vector<std::unique_ptr<ID3D12Resource>> planes;
        std::vector<uint8_t> host;
        for (const char* name : files) {
            const std::string path = dir + "/" + name;
            uint32_t w = 0, h = 0, levels = 0;
            CrychicThrowIfFailed(crychic_load_dds_rgba8_mips(path.c_str(), nullptr, 0, &w, &h, &levels));
            size_t bytes = 0;
            for (uint32_t k = 0, lw = w, lh = h; k < levels; ++k) { bytes += (size_t)lw * lh * 4; lw = lw > 1 ? lw >> 1 : 1; lh = lh > 1 ? lh >> 1 : 1; }
            host.resize(bytes);
            CrychicThrowIfFailed(crychic_load_dds_rgba8_mips(path.c_str(), host.data(), host.size(), &w, &h, &levels));
            planes.push_back(std::make_unique<ID3D12Resource>(bytes, ID3D12Resource::DEFAULT_HEAP));
            planes.back()->Upload(host.data(), bytes, s);
            mCommandList->Flush();                                      // `host` is reused for the next file
            tex.push_back(crychic_texture{ static_cast<const uint8_t*>(planes.back()->Data()), w, h, levels });
        }
        const std::string cubePath = dir + "/snowcube1024.dds";
        uint32_t dim = 0, cubeLevels = 0;
        const int rc = crychic_load_dds_cube_rgba8_mips(cubePath.c_str(), nullptr, 0, &dim, &cubeLevels);      // :1148-1151: the whole chain
        if (rc == 0) {
            host.resize(crychic_cube_chain_bytes(dim, cubeLevels));
            CrychicThrowIfFailed(crychic_load_dds_cube_rgba8_mips(cubePath.c_str(), host.data(), host.size(), &dim, &cubeLevels));
            auto cube = std::make_unique<ID3D12Resource>(host.size(), ID3D12Resource::DEFAULT_HEAP);
            cube->Upload(host.data(), host.size(), s);
            mCommandList->Flush();
            SetCubeMap(std::move(cube), dim, cubeLevels);
        } else if (requireCubeMap) {
            CrychicThrowIfFailed(rc);
        }
        mTextures = std::move(tex);
        mTexturePlanes = std::move(planes);
    }
    ID3D12GraphicsCommandList* CommandList() { return mCommandList.get(); }
    ID3D12Device* Device() { return md3dDevice.get(); }
    float AspectRatio() const { return (float)mClientWidth / (float)mClientHeight; }
    // The built scene, for a caller that edits it between Initialize() and the first Update(): item k of a layer (nullptr past the
    // end) and a material by name (nullptr if there is none).  After changing a material set its NumFramesDirty = gNumFrameResources.
    RenderItem* LayerItem(RenderLayer layer, size_t k) { auto& l = mRitemLayer[(int)layer]; return k < l.size() ? l[k] : nullptr; }
    Material* FindMaterial(const std::string& name) { auto it = mMaterials.find(name); return it == mMaterials.end() ? nullptr : it->second.get(); }

    bool mRunProducerPasses = true;   // false: the caller fills the input planes itself (tests, external producers)
    std::unique_ptr<ShadowMap> mShadowMap;
    std::unique_ptr<Ssao> mSsao;
    std::unique_ptr<DeferredShading> mDeferred;
    Camera mCamera;
    PassConstants mMainPassCB;  // index 0 of pass cbuffer (CRYCHIC.h:149)
    int mBlurCount = 3;         // CRYCHIC.cpp:221
    int mNumDirLights = 1;      // NUM_DIR_LIGHTS of the deferred shader (Common.hlsl:6-8)
    bool mPcfLiteral = true;    // Common.hlsl:305 evaluated as written
    bool mSkyEnabled = true;
    bool mFrustumCullingEnabled = true;   // CRYCHIC.h:188
    bool mFuseCameraPasses = true;        // false: DrawNormalsAndDepth and DrawGBuffer rasterise separately, as the reference records them
    UINT mShadowMapSize = 4096; // CRYCHIC.cpp:48-49
    DirectX::XMFLOAT4X4 mLightViews[MaxLights], mLightProjs[MaxLights], mShadowTransforms[MaxLights];  // CRYCHIC.h:166-170
    FrameResource* mCurrFrameResource = nullptr;

private:
    // ---- scene construction ---------------------------------------------------------------------------------------
    void BuildShapeGeometry()  // CRYCHIC.cpp:1250-1445: box + grid concatenated into one vertex / index buffer
    {
        uint32_t nbI = 0, ngI = 0;
        const int nbV = crychic_create_box(1.0f, 1.0f, 1.0f, 3, nullptr, 0, nullptr, 0, &nbI);         // :1253
        const int ngV = crychic_create_grid(20.0f, 30.0f, 60, 40, nullptr, 0, nullptr, 0, &ngI);       // :1254
        std::vector<crychic_vertex> v((size_t)nbV + ngV);
        std::vector<uint32_t> idx((size_t)nbI + ngI);
        CrychicThrowIfFailed(crychic_create_box(1.0f, 1.0f, 1.0f, 3, v.data(), nbV, idx.data(), nbI, &nbI));
        CrychicThrowIfFailed(crychic_create_grid(20.0f, 30.0f, 60, 40, v.data() + nbV, ngV, idx.data() + nbI, ngI, &ngI));
        auto geo = std::make_unique<MeshGeometry>();
        geo->Name = "shapeGeo";
        geo->VertexCount = (UINT)v.size(); geo->IndexCount = (UINT)idx.size();
        geo->VertexBufferGPU = std::make_unique<ID3D12Resource>(v.size() * sizeof(crychic_vertex), ID3D12Resource::DEFAULT_HEAP);
        geo->IndexBufferGPU = std::make_unique<ID3D12Resource>(idx.size() * 4, ID3D12Resource::DEFAULT_HEAP);
        geo->VertexBufferGPU->Upload(v.data(), v.size() * sizeof(crychic_vertex), mCommandList->Stream());
        geo->IndexBufferGPU->Upload(idx.data(), idx.size() * 4, mCommandList->Stream());
        mCommandList->Flush();
        auto bounds = [&](size_t first, size_t count) {                                                 // :1318-1337: min / max of the positions
            float lo[3] = { 3.4e38f, 3.4e38f, 3.4e38f }, hi[3] = { -3.4e38f, -3.4e38f, -3.4e38f };
            for (size_t k = first; k < first + count; ++k)
                for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], v[k].Pos[c]); hi[c] = std::max(hi[c], v[k].Pos[c]); }
            BoundingBox b;
            b.Center = { 0.5f * (lo[0] + hi[0]), 0.5f * (lo[1] + hi[1]), 0.5f * (lo[2] + hi[2]) };
            b.Extents = { 0.5f * (hi[0] - lo[0]), 0.5f * (hi[1] - lo[1]), 0.5f * (hi[2] - lo[2]) };
            return b;
        };
        geo->DrawArgs["box"] = SubmeshGeometry{ nbI, 0, 0, bounds(0, (size_t)nbV) };                   // :1271-1301
        geo->DrawArgs["grid"] = SubmeshGeometry{ ngI, nbI, nbV, bounds((size_t)nbV, (size_t)ngV) };
        mGeometries[geo->Name] = std::move(geo);
    }
    void BuildMaterials()  // CRYCHIC.cpp:1768-1821
    {
        auto add = [&](const char* name, int cb, int d, int n, DirectX::XMFLOAT4 alb, DirectX::XMFLOAT3 r0, float rough) {
            auto m = std::make_unique<Material>();
            m->Name = name; m->MatCBIndex = cb; m->DiffuseSrvHeapIndex = d; m->NormalSrvHeapIndex = n;
            m->DiffuseAlbedo = alb; m->FresnelR0 = r0; m->Roughness = rough;
            mMaterials[name] = std::move(m);
        };
        add("bricks0", 0, 0, 1, { 1.0f, 1.0f, 1.0f, 1.0f }, { 0.1f, 0.1f, 0.1f }, 0.3f);
        add("tile0", 1, 2, 3, { 0.9f, 0.9f, 0.9f, 1.0f }, { 0.2f, 0.2f, 0.2f }, 0.7f);
        add("mirror0", 2, 4, 5, { 0.0f, 0.0f, 0.0f, 1.0f }, { 0.98f, 0.97f, 0.95f }, 0.1f);
        add("skullMat", 3, 4, 5, { 1.0f, 1.0f, 1.0f, 1.0f }, { 0.6f, 0.6f, 0.6f }, 0.8f);
        add("sky", 4, 6, 7, { 1.0f, 1.0f, 1.0f, 1.0f }, { 0.1f, 0.1f, 0.1f }, 1.0f);
    }
    static DirectX::XMFLOAT4X4 ScaleTranslate(float s, float tx, float ty, float tz)   // XMMatrixScaling * XMMatrixTranslation
    {
        return DirectX::XMFLOAT4X4{ { { s, 0, 0, 0 }, { 0, s, 0, 0 }, { 0, 0, s, 0 }, { tx, ty, tz, 1 } } };
    }
    void AddBoxAndGrid(RenderLayer layer, int boxMaterialModulo, UINT gridMaterial)
    {
        MeshGeometry* geo = mGeometries["shapeGeo"].get();
        auto box = std::make_unique<RenderItem>();
        box->itemIndex = mItemIndex++;
        box->Geo = geo;
        box->IndexCount = geo->DrawArgs["box"].IndexCount;
        box->StartIndexLocation = geo->DrawArgs["box"].StartIndexLocation;
        box->BaseVertexLocation = geo->DrawArgs["box"].BaseVertexLocation;
        box->Bounds = geo->DrawArgs["box"].Bounds;                                                   // :1882
        box->Instances.resize(100);
        box->InstanceCount = 100;
        for (int i = 0; i < 10; ++i)
            for (int j = 0; j < 10; ++j) {                                                            // :2338-2346, 2398-2406
                box->Instances[i * 10 + j].World = ScaleTranslate(1.6f, (-5 + i) * 5.0f, 0.8f, (-5 + j) * 5.0f);
                box->Instances[i * 10 + j].MaterialIndex = (UINT)(i % boxMaterialModulo);
            }
        mInstanceCounts.push_back(100);
        mRitemLayer[(int)layer].push_back(box.get());
        mAllRitems.push_back(std::move(box));
        auto grid = std::make_unique<RenderItem>();
        grid->itemIndex = mItemIndex++;
        grid->Geo = geo;
        grid->IndexCount = geo->DrawArgs["grid"].IndexCount;
        grid->StartIndexLocation = geo->DrawArgs["grid"].StartIndexLocation;
        grid->BaseVertexLocation = geo->DrawArgs["grid"].BaseVertexLocation;
        grid->Bounds = geo->DrawArgs["grid"].Bounds;                                                 // :1930
        grid->Instances.resize(1);
        grid->InstanceCount = 1;
        grid->Instances[0].World = ScaleTranslate(3.0f, 0.0f, 0.0f, 0.0f);                            // :2371, 2431
        grid->Instances[0].MaterialIndex = gridMaterial;
        mInstanceCounts.push_back(1);
        mRitemLayer[(int)layer].push_back(grid.get());
        mAllRitems.push_back(std::move(grid));
    }
    void BuildCascadeShadowRenderItems() { AddBoxAndGrid(RenderLayer::Opaque, 2, 3); }               // CRYCHIC.cpp:2322-2375 (sky / debug quad are not drawn by the deferred path's producers)
    void BuildCascadeShadowRenderItemsWithShadow() { AddBoxAndGrid(RenderLayer::OpaqueShadow, 3, 1); }  // :2380-2435

    void BuildFrameResources()  // CRYCHIC.cpp:1759-1766: 1 main + 12 shadow pass slots
    {
        for (int i = 0; i < gNumFrameResources; ++i) {
            mFrameResources.push_back(std::make_unique<FrameResource>(md3dDevice.get(), 1 + 12, mInstanceCounts, (UINT)mAllRitems.size(),
                                                                      (UINT)mMaterials.size()));
            CrychicHipThrowIfFailed(hipEventCreateWithFlags(&mFrameResources.back()->FenceEvent, hipEventDisableTiming));
        }
    }
    static DirectX::XMFLOAT4X4 Transposed(const DirectX::XMFLOAT4X4& a)
    {
        DirectX::XMFLOAT4X4 t;
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) t.m[i][j] = a.m[j][i];
        return t;
    }
    void UpdateInstanceData(const GameTimer&)  // CRYCHIC.cpp:515-564: only instances that pass the frustum test reach the instance buffer
    {
        std::vector<uint8_t> visible;
        for (auto& ri : mAllRitems) {
            auto* buf = mCurrFrameResource->InstanceBuffers[ri->itemIndex].get();
            visible.assign(ri->Instances.size(), 1);
            if (mFrustumCullingEnabled && !ri->Instances.empty()) {                                   // :543-544
                std::vector<float> worlds(ri->Instances.size() * 16);
                for (size_t k = 0; k < ri->Instances.size(); ++k) std::memcpy(&worlds[16 * k], ri->Instances[k].World.m, 64);
                const float c[3] = { ri->Bounds.Center.x, ri->Bounds.Center.y, ri->Bounds.Center.z };
                const float e[3] = { ri->Bounds.Extents.x, ri->Bounds.Extents.y, ri->Bounds.Extents.z };
                CrychicThrowIfFailed(std::min(0, crychic_frustum_cull(&mCamera.Raw(), c, e, worlds.data(), (uint32_t)ri->Instances.size(), visible.data())));
            }
            int n = 0;
            for (size_t k = 0; k < ri->Instances.size(); ++k) {
                if (!visible[k]) continue;
                const InstanceData& src = ri->Instances[k];
                InstanceData data;
                data.World = Transposed(src.World);                                                   // :546
                data.TexTransform = Transposed(src.TexTransform);                                     // :547
                data.MaterialIndex = src.MaterialIndex;
                buf->CopyData(n++, data);
            }
            ri->InstanceCount = (UINT)n;
        }
    }
    void UpdateMaterialBuffer(const GameTimer&)  // CRYCHIC.cpp:566-592
    {
        auto* buf = mCurrFrameResource->MaterialBuffer.get();
        for (auto& e : mMaterials) {
            Material* mat = e.second.get();
            if (mat->NumFramesDirty > 0) {
                MaterialData d;
                d.DiffuseAlbedo = mat->DiffuseAlbedo; d.FresnelR0 = mat->FresnelR0; d.Roughness = mat->Roughness;
                d.MatTransform = Transposed(mat->MatTransform);
                d.DiffuseMapIndex = (UINT)mat->DiffuseSrvHeapIndex; d.NormalMapIndex = (UINT)mat->NormalSrvHeapIndex;
                buf->CopyData(mat->MatCBIndex, d);                                                    // Metalness keeps its default 0.5 (Q5)
                mat->NumFramesDirty--;
            }
        }
    }
    void UpdateShadowPassCB(const GameTimer&)  // CRYCHIC.cpp:870-901: slots 1..12, of which cascades 0..3 are meaningful
    {
        for (int i = 0; i < 4; ++i) {
            PassConstants cb;
            ViewProjTransposed(&mLightViews[i].m[0][0], &mLightProjs[i].m[0][0], &cb.ViewProj.m[0][0]);
            for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { cb.View.m[c][r] = mLightViews[i].m[r][c]; cb.Proj.m[c][r] = mLightProjs[i].m[r][c]; }
            cb.RenderTargetSize = { (float)mShadowMap->Width(), (float)mShadowMap->Height() };
            cb.InvRenderTargetSize = { 1.0f / mShadowMap->Width(), 1.0f / mShadowMap->Height() };
            mCurrFrameResource->PassCB->CopyData(1 + i, cb);                                          // :897-898
        }
    }

    // ---- producer passes --------------------------------------------------------------------------------------------
    // view * proj (row-major 4 x 4 each), stored transposed as the pass constants hold it.  The shadow maps are compared bit for
    // bit: the sum runs over k = 0 .. 3 in this order.
    static void ViewProjTransposed(const float* view, const float* proj, float* out)
    {
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) {
            float acc = 0.0f;
            for (int k = 0; k < 4; ++k) acc += view[4 * r + k] * proj[4 * k + c];
            out[4 * c + r] = acc;
        }
    }
    std::vector<crychic_draw_item> DrawItems(const std::vector<RenderItem*>& ritems)  // CRYCHIC::DrawRenderItems, CRYCHIC.cpp:2438-2475
    {
        std::vector<crychic_draw_item> out;
        mSceneTriangles = 0;
        for (RenderItem* ri : ritems) {
            crychic_draw_item d = {};
            d.vertices_dev = static_cast<const crychic_vertex*>(ri->Geo->VertexBufferGPU->Data());
            d.vertexCount = ri->Geo->VertexCount;
            d.indices_dev = static_cast<const uint32_t*>(ri->Geo->IndexBufferGPU->Data());
            d.indexCount = ri->IndexCount; d.startIndexLocation = ri->StartIndexLocation; d.baseVertexLocation = ri->BaseVertexLocation;
            d.instances_dev = reinterpret_cast<const crychic_instance_data*>(mCurrFrameResource->InstanceBuffers[ri->itemIndex]->Resource()->Data());
            d.instanceCount = ri->InstanceCount;
            out.push_back(d);
            mSceneTriangles += (uint64_t)(ri->IndexCount / 3) * ri->InstanceCount;
        }
        return out;
    }
    void* RasterWorkspace(uint64_t triangles, UINT W, UINT H, size_t* bytes)
    {
        *bytes = crychic_raster_workspace_bytes(triangles, W, H);
        if (!mRasterWorkspace || mRasterWorkspace->Bytes() < *bytes) mRasterWorkspace = std::make_unique<ID3D12Resource>(*bytes, ID3D12Resource::DEFAULT_HEAP);
        return mRasterWorkspace->Data();
    }
    void DrawSceneToShadowMap()  // CRYCHIC.cpp:2477-2510 (the reference loops 6 times; cascades 0..3 carry data, Q8)
    {
        auto items = DrawItems(mRitemLayer[(int)RenderLayer::OpaqueShadow]);
        size_t bytes;
        void* ws = RasterWorkspace(4 * mSceneTriangles, mShadowMap->Width(), mShadowMap->Height(), &bytes);
        // the four cascades' pass constants sit in consecutive 256-byte-aligned slots of the upload buffer; gather them
        crychic_pass_constants cbs[4];
        uint32_t* targets[4];
        for (int i = 0; i < 4; ++i) {
            std::memcpy(&cbs[i], &mCurrFrameResource->PassCB->Element(1 + i), sizeof cbs[i]);
            targets[i] = static_cast<uint32_t*>(mShadowMap->Resource(i)->Data());
        }
        CrychicThrowIfFailed(crychic_draw_scene_to_shadow_maps(md3dDevice->Ctx(), cbs, 4, items.data(), (uint32_t)items.size(), targets,
                                                               mShadowMap->Width(), 10000, 2.0f, ws, bytes, mCommandList->Stream()));  // bias: :1601-1603
        if (mSpotShadowCount > 0) DrawSpotShadowMaps(items);
        if (mPointShadowCount > 0) DrawPointShadowMaps(items);
    }
    void DrawSpotShadowMaps(const std::vector<crychic_draw_item>& items)
    {
        size_t bytes;
        // the shadowed spot lights' maps (slots 4..11): one more pass of the same rasteriser, ViewProj = lightView * lightProj
        crychic_pass_constants scbs[CRYCHIC_MAX_SPOT_SHADOWS];
        uint32_t* stargets[CRYCHIC_MAX_SPOT_SHADOWS];
        for (uint32_t k = 0; k < mSpotShadowCount; ++k) {
            std::memset(&scbs[k], 0, sizeof scbs[k]);
            ViewProjTransposed(&mLightViews[4 + k].m[0][0], &mLightProjs[4 + k].m[0][0], scbs[k].ViewProj);
            stargets[k] = static_cast<uint32_t*>(mSpotShadowMaps[k]->Data());
        }
        void* sws = RasterWorkspace((uint64_t)mSpotShadowCount * mSceneTriangles, mSpotShadowDim, mSpotShadowDim, &bytes);
        CrychicThrowIfFailed(crychic_draw_scene_to_shadow_maps(md3dDevice->Ctx(), scbs, mSpotShadowCount, items.data(), (uint32_t)items.size(),
                                                               stargets, mSpotShadowDim, 10000, 2.0f, sws, bytes, mCommandList->Stream()));
    }
    void DrawPointShadowMaps(const std::vector<crychic_draw_item>& items)
    {
        // the shadowed point lights' faces: the same rasteriser, ViewProj = lightView[f] * lightProj, at most 12 faces (two lights) per call
        size_t bytes;
        const uint32_t nFaces = 6u * mPointShadowCount, perCall = 12u;
        void* pws = RasterWorkspace((uint64_t)(nFaces < perCall ? nFaces : perCall) * mSceneTriangles, mPointShadowDim, mPointShadowDim, &bytes);
        for (uint32_t first = 0; first < nFaces; first += perCall) {
            const uint32_t n = nFaces - first < perCall ? nFaces - first : perCall;
            crychic_pass_constants pcbs[12];
            uint32_t* ptargets[12];
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t k = (first + i) / 6u, face = (first + i) % 6u;
                std::memset(&pcbs[i], 0, sizeof pcbs[i]);
                ViewProjTransposed(mPointViews[k][face], mPointProjs[k], pcbs[i].ViewProj);
                ptargets[i] = static_cast<uint32_t*>(mPointShadowMaps[k]->Data()) + (size_t)face * mPointShadowDim * mPointShadowDim;
            }
            CrychicThrowIfFailed(crychic_draw_scene_to_shadow_maps(md3dDevice->Ctx(), pcbs, n, items.data(), (uint32_t)items.size(), ptargets,
                                                                   mPointShadowDim, 10000, 2.0f, pws, bytes, mCommandList->Stream()));
        }
    }
    void DrawNormalsAndDepth()  // CRYCHIC.cpp:2512-2543
    {
        auto items = DrawItems(mRitemLayer[(int)RenderLayer::Opaque]);
        size_t bytes;
        void* ws = RasterWorkspace(mSceneTriangles, mClientWidth, mClientHeight, &bytes);
        const PassConstants& cb = mCurrFrameResource->PassCB->Element(0);
        CrychicThrowIfFailed(crychic_draw_normals_and_depth(md3dDevice->Ctx(), reinterpret_cast<const crychic_pass_constants*>(&cb), items.data(),
                                                            (uint32_t)items.size(), mSsao->NormalMap()->Data(),
                                                            static_cast<uint32_t*>(mDepthStencilBuffer->Data()), mClientWidth, mClientHeight, ws, bytes,
                                                            mCommandList->Stream()));
    }
    void DrawGBuffer() { DrawCameraPass(nullptr); }  // CRYCHIC.cpp:2545-2571
    // DrawNormalsAndDepth + DrawGBuffer: same items, same ViewProj, same visibility -> one rasterisation
    void DrawNormalsDepthAndGBuffer() { DrawCameraPass(mSsao->NormalMap()->Data()); }
    void DrawCameraPass(void* normalMap)  // the G-buffer and depth, with the view normals too when there is a map for them
    {
        auto items = DrawItems(mRitemLayer[(int)RenderLayer::Opaque]);
        size_t bytes;
        void* ws = RasterWorkspace(mSceneTriangles, mClientWidth, mClientHeight, &bytes);
        const PassConstants& cb = mCurrFrameResource->PassCB->Element(0);
        const auto* mats = reinterpret_cast<const crychic_material_data*>(mCurrFrameResource->MaterialBuffer->Resource()->Data());
        // the scissor rectangle of this pass (CRYCHIC.cpp:2547-2548) is this GPU's strip when the frame is shared (SetStrip / JoinNode,
        // which refuse an empty one); FormatFlags() marks the half4 planes among G0..G2, 0 = float4 throughout
        CrychicThrowIfFailed(crychic_draw_gbuffer_formats(md3dDevice->Ctx(), reinterpret_cast<const crychic_pass_constants*>(&cb), items.data(),
                                                          (uint32_t)items.size(), mats, (uint32_t)mMaterials.size(),
                                                          mTextures.empty() ? nullptr : mTextures.data(), (uint32_t)mTextures.size(), normalMap,
                                                          mDeferred->Resource(0)->Data(), mDeferred->Resource(1)->Data(), mDeferred->Resource(2)->Data(),
                                                          mDeferred->FormatFlags(), static_cast<uint32_t*>(mDepthStencilBuffer->Data()), mClientWidth,
                                                          mClientHeight, mStripRow0, mWholeFrame ? mClientHeight : mStripRows, ws, bytes,
                                                          mCommandList->Stream()));
    }
    void ApplyDecals()  // the decals of SetDecals into this GPU's rows of the G-buffer the camera pass has just written
    {
        const PassConstants& cb = mCurrFrameResource->PassCB->Element(0);
        CrychicThrowIfFailed(crychic_apply_decals(md3dDevice->Ctx(), reinterpret_cast<const crychic_pass_constants*>(&cb),
                                                  static_cast<const uint32_t*>(mDepthStencilBuffer->Data()), mDeferred->Resource(0)->Data(),
                                                  mDeferred->Resource(1)->Data(), mDeferred->Resource(2)->Data(), mDeferred->FormatFlags(),
                                                  static_cast<const crychic_decal*>(mDecals->Data()), mDecalCount,
                                                  mDecalTextures.empty() ? nullptr : mDecalTextures.data(), (uint32_t)mDecalTextures.size(), mClientWidth,
                                                  mClientHeight, mStripRow0, mWholeFrame ? mClientHeight : mStripRows, mCommandList->Stream()));
    }
    void UpdateCascadeShadowTransform(const GameTimer&)  // CRYCHIC.cpp:634-815
    {
        const float ld[3] = { mBaseLightDirections[0].x, mBaseLightDirections[0].y, mBaseLightDirections[0].z };  // :726
        float lv[4][16], lp[4][16], st[4][16];
        CrychicThrowIfFailed(crychic_update_cascade_shadow_transform(&mCamera.Raw(), ld, mShadowMap->Width(), lv, lp, st));
        for (int i = 0; i < 4; ++i) {
            std::memcpy(&mLightViews[i], lv[i], 64); std::memcpy(&mLightProjs[i], lp[i], 64); std::memcpy(&mShadowTransforms[i], st[i], 64);
        }
    }
    void UpdateSpotShadowTransforms()  // SetSpotShadows: the light, projection and shadow transform of slots 4 .. 4 + count - 1
    {
        for (uint32_t k = 0; k < mSpotShadowCount; ++k) {
            float v[16], p[16], t[16];
            CrychicThrowIfFailed(crychic_update_spot_shadow_transform(reinterpret_cast<const crychic_light*>(&mSpotHost[k]), mSpotShadowFovY,
                                                                      mSpotShadowZNear, v, p, t));
            std::memcpy(&mLightViews[4 + k], v, 64); std::memcpy(&mLightProjs[4 + k], p, 64); std::memcpy(&mShadowTransforms[4 + k], t, 64);
        }
    }
    void UpdatePointShadowTransforms()  // SetPointShadows / SetLocalLights: the faces, projection and shadow projection of each shadowed point light
    {
        for (uint32_t k = 0; k < mPointShadowCount; ++k)
            CrychicThrowIfFailed(crychic_update_point_shadow_transforms(reinterpret_cast<const crychic_light*>(&mPointHost[k]), mPointShadowDim,
                                                                        mPointShadowZNear, mPointViews[k], mPointProjs[k], mPointShadowProjs[k]));
    }
    void UpdateMainPassCB(const GameTimer& gt)  // CRYCHIC.cpp:817-868
    {
        float st[4][16], dirs[3][3];
        for (int i = 0; i < 4; ++i) std::memcpy(st[i], &mShadowTransforms[i], 64);
        for (int i = 0; i < 3; ++i) { dirs[i][0] = mRotatedLightDirections[i].x; dirs[i][1] = mRotatedLightDirections[i].y; dirs[i][2] = mRotatedLightDirections[i].z; }
        CrychicThrowIfFailed(crychic_update_main_pass_cb(&mCamera.Raw(), mClientWidth, mClientHeight, st, dirs,
                                                         reinterpret_cast<crychic_pass_constants*>(&mMainPassCB)));
        if (mMotionBlur) {
            // the unjittered ViewProj built above becomes this frame's, what was this frame's the previous one's (its own on a first frame)
            std::memcpy(mMbViewProj[1], mMbFirst ? reinterpret_cast<const float*>(&mMainPassCB.ViewProj) : mMbViewProj[0], 64);
            std::memcpy(mMbViewProj[0], &mMainPassCB.ViewProj, 64);
            mMbFirst = false;
        }
        if (mTemporalAA || mTemporalUpscale) {
            // the unjittered ViewProj built above becomes this frame's, what was this frame's the previous one's (its own on a reset
            // frame); then the constants again with the projection shifted by the frame's jitter
            std::memcpy(mTaaViewProj[1], (mTemporalAA ? mTaaReset : mTuReset) ? reinterpret_cast<const float*>(&mMainPassCB.ViewProj) : mTaaViewProj[0], 64);
            std::memcpy(mTaaViewProj[0], &mMainPassCB.ViewProj, 64);
            CrychicThrowIfFailed(crychic_update_main_pass_cb_jittered(&mCamera.Raw(), mClientWidth, mClientHeight, st, dirs, mTaaJitter[0], mTaaJitter[1],
                                                                      reinterpret_cast<crychic_pass_constants*>(&mMainPassCB)));
        }
        const CRYCHIC& L = mOwner ? *mOwner : *this;                                                // a capture's probe: its owner's spot shadows
        for (uint32_t k = 0; k < L.mSpotShadowCount; ++k)                                           // slots 4..11, transposed like :826-830
            for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) mMainPassCB.ShadowTransforms[4 + k].m[c][r] = L.mShadowTransforms[4 + k].m[r][c];
        mMainPassCB.TotalTime = gt.TotalTime();
        mMainPassCB.DeltaTime = gt.DeltaTime();
        mCurrFrameResource->PassCB->CopyData(0, mMainPassCB);                                       // :866-867
    }
    void UpdateSsaoCB(const GameTimer&)  // CRYCHIC.cpp:903-937
    {
        SsaoConstants ssaoCB;
        DirectX::XMFLOAT4 off[14];
        mSsao->GetOffsetVectors(off);                                                               // :920
        float o[14][4];
        for (int i = 0; i < 14; ++i) { o[i][0] = off[i].x; o[i][1] = off[i].y; o[i][2] = off[i].z; o[i][3] = off[i].w; }
        if (mTemporalAA || mTemporalUpscale)
            CrychicThrowIfFailed(crychic_update_ssao_cb_jittered(&mCamera.Raw(), mClientWidth, mClientHeight, o, mTaaJitter[0], mTaaJitter[1],
                                                                 reinterpret_cast<crychic_ssao_constants*>(&ssaoCB)));
        else
            CrychicThrowIfFailed(crychic_update_ssao_cb(&mCamera.Raw(), mClientWidth, mClientHeight, o, reinterpret_cast<crychic_ssao_constants*>(&ssaoCB)));
        mCurrFrameResource->SsaoCB->CopyData(0, ssaoCB);                                            // :935-936
    }

    std::unordered_map<std::string, std::unique_ptr<MeshGeometry>> mGeometries;      // CRYCHIC.h:123-125
    std::unordered_map<std::string, std::unique_ptr<Material>> mMaterials;
    std::vector<crychic_texture> mTextures;                                           // gTextureMaps (row f4 loads the DDS files; empty = white / flat)
    std::vector<std::unique_ptr<ID3D12Resource>> mTexturePlanes;                      // the device copies mTextures points into (LoadTextures)
    std::vector<std::unique_ptr<RenderItem>> mAllRitems;                              // CRYCHIC.h:132-135
    std::vector<RenderItem*> mRitemLayer[(int)RenderLayer::Count];
    std::vector<int> mInstanceCounts;                                                 // CRYCHIC.h:183
    UINT mItemIndex = 0;
    uint64_t mSceneTriangles = 0;
    std::unique_ptr<ID3D12Resource> mRasterWorkspace;
    std::unique_ptr<ID3D12Device> md3dDevice;
    std::unique_ptr<ID3D12GraphicsCommandList> mCommandList;
    std::vector<std::unique_ptr<FrameResource>> mFrameResources;
    int mCurrFrameResourceIndex = 0;
    UINT64 mCurrentFence = 0;
    crychic_comm* mComm = nullptr;            // set by JoinNode: this GPU renders a strip and gathers the others'
    std::vector<uint32_t> mStripBounds;       // nranks x {row0, rows}; empty = crychic_strip_rows
    UINT mStripRow0 = 0, mStripRows = 0;      // this GPU's rows when the frame is shared
    UINT mExchangeParts = 1;                  // SetExchangeParts
    bool mWholeFrame = true;
    bool mFog = false;                        // SetFog
    crychic_fog_params mFogParams = {};
    std::unique_ptr<ID3D12Resource> mDecals;  // SetDecals: the device array
    uint32_t mDecalCount = 0;
    std::vector<crychic_texture> mDecalTextures;
    bool mScreenSpaceReflections = false;     // SetScreenSpaceReflections
    crychic_ssr_params mSsrParams = {};
    std::unique_ptr<ID3D12Resource> mBackBufferSSR;  // the frame behind the screen-space reflections, while mScreenSpaceReflections
    bool mSsrGloss = false;                   // SetScreenSpaceReflectionGloss
    crychic_ssr_gloss_params mSsrGlossParams = {};
    std::unique_ptr<ID3D12Resource> mSsrPyramid;     // the lit frame's pyramid: the frame's size at the most levels, so any parameters fit
    void AllocateSsrPyramid()
    {
        const size_t need = crychic_ssr_pyramid_bytes(mClientWidth, mClientHeight, CRYCHIC_SSR_GLOSS_MAX_LEVELS);
        mSsrPyramid = std::make_unique<ID3D12Resource>(need < 16 ? 16 : need, ID3D12Resource::DEFAULT_HEAP);
    }
    bool mDepthOfField = false;               // SetDepthOfField
    crychic_dof_params mDofParams = {};
    std::unique_ptr<ID3D12Resource> mBackBufferDoF;  // the frame behind the depth-of-field pass, while mDepthOfField
    bool mBloom = false;                      // SetBloom
    crychic_bloom_params mBloomParams = {};
    std::unique_ptr<ID3D12Resource> mBackBufferBloom;  // the frame behind the bloom pass, while mBloom
    std::unique_ptr<ID3D12Resource> mBloomWorkspace;   // its pyramid: the frame's size at the most levels, so any parameters fit
    void AllocateBloom()
    {
        mBackBufferBloom = FinalPlane();
        mBloomWorkspace = std::make_unique<ID3D12Resource>(crychic_bloom_workspace_bytes(FinalWidth(), FinalHeight(), CRYCHIC_BLOOM_MAX_LEVELS),
                                                           ID3D12Resource::DEFAULT_HEAP);
    }
    bool mColourGrade = false;                // SetColourGrade / SetColourGradeLut / LoadColourGradeLut
    uint32_t mGradeN = 0;
    std::unique_ptr<ID3D12Resource> mGradeLut;         // the table, uploaded by the setter
    std::unique_ptr<ID3D12Resource> mBackBufferGrade;  // the graded frame, while mColourGrade
    bool mSharpening = false;                 // SetSharpening
    crychic_sharpen_params mSharpenParams = {};
    std::unique_ptr<ID3D12Resource> mBackBufferSharp;  // the sharpened frame, while mSharpening
    bool mTemporalAA = false;                 // SetTemporalAA
    crychic_taa_params mTaaParams = {};
    std::unique_ptr<ID3D12Resource> mBackBufferTAA;    // the resolved frame, while mTemporalAA
    std::unique_ptr<ID3D12Resource> mTaaHistory[2];    // the history planes: [mTaaHistoryIndex] is read by the next Draw, the other written
    int mTaaHistoryIndex = 0;
    bool mTaaReset = true;                    // the next frame does not read the history
    uint32_t mTaaFrameIndex = 0;              // the jitter sequence's running index
    float mTaaJitter[2] = { 0.0f, 0.0f };     // this frame's offset in pixels
    float mTaaViewProj[2][16] = {};           // the unjittered ViewProj of this frame and of the previous one (stored transposed)
    void AllocateTemporalAA()
    {
        mBackBufferTAA = FramePlane();
        for (auto& h : mTaaHistory) h = std::make_unique<ID3D12Resource>(crychic_taa_history_bytes(mClientWidth, mClientHeight), ID3D12Resource::DEFAULT_HEAP);
        mTaaHistoryIndex = 0;
        mTaaReset = true;
    }
    void SetTemporalAA(bool on, const crychic_taa_params& q)
    {
        if (q.blend == 0u || q.blend > 256u || (q.flags & ~(CRYCHIC_TAA_RESET | CRYCHIC_TAA_NO_CLAMP)) ||
            (q.reserved[0] | q.reserved[1] | q.reserved[2] | q.reserved[3] | q.reserved[4] | q.reserved[5]))
            throw CrychicException(CRYCHIC_E_INVALID_ARG, "CRYCHIC::SetTemporalAA (blend 1 .. 256, flags RESET | NO_CLAMP, reserved 0)", __FILE__, __LINE__);
        mCommandList->Flush();                                  // a frame in flight may still write the buffers released below
        const bool was = mTemporalAA;
        mTemporalAA = on;
        mTaaParams = q;
        if (on && !was) { AllocateTemporalAA(); mTaaFrameIndex = 0; }
        if (!on) { mBackBufferTAA.reset(); mTaaHistory[0].reset(); mTaaHistory[1].reset(); }
    }
    bool mTemporalUpscale = false;            // SetTemporalUpscale
    crychic_taa_upscale_params mTuParams = {};
    uint32_t mTuWidth = 0, mTuHeight = 0;     // the display size
    std::unique_ptr<ID3D12Resource> mBackBufferUpscaled;   // the resolved frame of the display size, while mTemporalUpscale
    std::unique_ptr<ID3D12Resource> mTuHistory[2];     // as mTaaHistory, of the display size
    int mTuHistoryIndex = 0;
    bool mTuReset = true;                     // the next frame does not read the history: apart from mTaaReset
    void AllocateTemporalUpscale()
    {
        mBackBufferUpscaled = FinalPlane();
        for (auto& h : mTuHistory) h = std::make_unique<ID3D12Resource>(crychic_taa_history_bytes(mTuWidth, mTuHeight), ID3D12Resource::DEFAULT_HEAP);
        mTuHistoryIndex = 0;
        mTuReset = true;
    }
    bool mMotionBlur = false;                 // SetMotionBlur
    crychic_motion_blur_params mMbParams = {};
    std::unique_ptr<ID3D12Resource> mBackBufferMB;     // the frame behind the motion blur, while mMotionBlur
    std::unique_ptr<ID3D12Resource> mMbWorkspace;      // its velocity and tile planes
    bool mMbFirst = true;                     // the next Update has no previous camera
    float mMbViewProj[2][16] = {};            // the unjittered ViewProj of this frame and of the previous one (stored transposed)
    void AllocateMotionBlur()
    {
        mBackBufferMB = FramePlane();
        mMbWorkspace = std::make_unique<ID3D12Resource>(crychic_motion_blur_workspace_bytes(mClientWidth, mClientHeight), ID3D12Resource::DEFAULT_HEAP);
        mMbFirst = true;
    }
    bool mAntiAliasing = false;               // SetAntiAliasing
    crychic_aa_params mAAParams = {};
    std::unique_ptr<ID3D12Resource> mBackBufferAA;   // the anti-aliased frame, while mAntiAliasing
    std::unique_ptr<ID3D12Resource> FramePlane() const      // a plane of the frame's size at four bytes a pixel: RGBA8, or the depth plane
    {
        return std::make_unique<ID3D12Resource>((size_t)mClientWidth * mClientHeight * 4, ID3D12Resource::DEFAULT_HEAP);
    }
    std::unique_ptr<ID3D12Resource> FinalPlane() const      // an RGBA8 plane of the finished frame's size: the display's behind the temporal upsampling
    {
        return std::make_unique<ID3D12Resource>((size_t)FinalWidth() * FinalHeight() * 4, ID3D12Resource::DEFAULT_HEAP);
    }
    ID3D12Resource* FinalFrame() const           // where Draw leaves the finished frame: the buffer of the last stage that is on
    {
        return (mAntiAliasing ? mBackBufferAA : mColourGrade ? mBackBufferGrade : mBloom ? mBackBufferBloom : mMotionBlur ? mBackBufferMB : mDepthOfField ? mBackBufferDoF
                : mSharpening ? mBackBufferSharp : mTemporalAA ? mBackBufferTAA : mTemporalUpscale ? mBackBufferUpscaled : mScreenSpaceReflections ? mBackBufferSSR : mBackBuffer).get();
    }
    std::unique_ptr<ID3D12Resource> mDepthStencilBuffer, mBackBuffer, mCubeMap;
    std::unique_ptr<ID3D12Resource> mPointLights, mSpotLights;   // SetLocalLights
    uint32_t mNumPointLights = 0, mNumSpotLights = 0;
    std::vector<Light> mSpotHost;                                         // SetLocalLights' spot list, for the shadow transforms
    std::vector<std::unique_ptr<ID3D12Resource>> mSpotShadowMaps;         // SetSpotShadows
    uint32_t mSpotShadowCount = 0, mSpotShadowDim = 0;
    float mSpotShadowFovY = 0.0f, mSpotShadowZNear = 0.0f;
    std::vector<Light> mPointHost;                                        // SetLocalLights' point list, for the face transforms
    std::vector<std::unique_ptr<ID3D12Resource>> mPointShadowMaps;        // SetPointShadows: six faces per light
    uint32_t mPointShadowCount = 0, mPointShadowDim = 0;
    float mPointShadowZNear = 0.0f;
    float mPointViews[CRYCHIC_MAX_POINT_SHADOWS][6][16] = {}, mPointProjs[CRYCHIC_MAX_POINT_SHADOWS][16] = {};
    float mPointShadowProjs[CRYCHIC_MAX_POINT_SHADOWS][16] = {};
    UINT mCubeMapSize = 0, mCubeMapLevels = 1;
    bool mGlossyReflections = false;                // SetGlossyReflections
    bool mEnvironmentAmbient = false;               // SetEnvironmentAmbient
    bool mCubeMapHasTail = false;                   // SetCubeMap(..., hasTail): the environment tail follows the bound cube map
    bool mEnvironmentSpecular = false;              // SetEnvironmentSpecular
    bool mCubeMapHasTable = false;                  // SetCubeMap(..., hasTable): the environment BRDF table follows the environment tail
    bool mProbeBoxSet = false;                      // SetReflectionProbeBox / ClearReflectionProbeBox
    bool mCubeMapHasProbe = false;                  // the bound cube map's environment tail holds the probe volume
    bool mHaveCapturePos = false;                   // the bound cube map is CaptureEnvironment's, taken at mCapturePos
    float mProbeBoxMin[3] = {}, mProbeBoxMax[3] = {}, mCapturePos[3] = {};
    std::unique_ptr<ID3D12Resource> mCaptureBoxChain;   // CaptureEnvironment with glossy reflections: the captured box chain, kept
    bool mFollowSun = false;                        // SetProceduralSky
    crychic_sky_params mSkyParams = {};             // SetProceduralSky's, and from the last FollowSun on with the sun it rendered
    const ID3D12Resource* mSkyOf = nullptr;         // the cube map FollowSun bound last (nullptr: none yet, or the parameters changed)
    UINT mSkyRenders = 0;
    UINT mClientWidth, mClientHeight;
    float mLightRotationAngle = 0.0f;
    DirectX::XMFLOAT3 mBaseLightDirections[3] = { { 0.57735f, -0.57735f, 0.57735f }, { -0.57735f, -0.57735f, 0.57735f }, { 0.0f, -0.707f, -0.707f } };  // CRYCHIC.h:173-177
    DirectX::XMFLOAT3 mRotatedLightDirections[3];
    int mDeviceOrdinal = 0;
    GameTimer mLastTimer;                           // the timer of the last Update
    const CRYCHIC* mOwner = nullptr;                // CaptureEnvironment, on the probe: whose cube map, local lights and shadow maps Draw reads
    std::unique_ptr<ID3D12Resource> mSpareCubeMap;  // CaptureEnvironment: the cube map the last capture replaced, the next one's destination
    uint8_t* mRenderTarget = nullptr;               // CaptureEnvironment, on the probe: the face the lighting pass writes (not owned)
    std::unique_ptr<CRYCHIC> mProbe;                // CaptureEnvironment's dim x dim renderer, kept across captures; declared last: destroyed first
};
