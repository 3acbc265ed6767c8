"""Python mirror of the reference's pass objects over the C ABI.

Class and method names follow the reference (Ssao.h:10-125, DeferredShading.h:4-45, ShadowMap.h:4-47,
CRYCHIC.h:56-190) so that the parity tests read like calls into the reference; D3D12 handles become torch
tensors that own HBM (PyTorch is used for device memory and streams only -- every pixel is computed by
libcrychic_hip.so).
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import (AAParams, CrychicError, FogParams, SkyParams, SsrParams, SsrGlossParams, DofParams, BloomParams, GradeParams, SharpenParams, TaaParams, TaaUpscaleParams, MotionBlurParams, DrawItem, FrameDesc, Light, PassConstants, PassTimes, PointShadows, SpotShadows, SsaoConstants, Texture,
                   check, lib)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _check_chain(who, chain, nbytes):
    if chain.dtype != torch.uint8 or not chain.is_contiguous() or chain.numel() < nbytes:
        raise CrychicError(-1, "%s: chain must be a contiguous uint8 device tensor of at least %d bytes" % (who, nbytes))


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Context:
    """One GPU, one context (D3DApp::InitDirect3D, Common/d3dApp.cpp:415-479)."""

    def __init__(self, device_ordinal=0):
        self.handle = C.c_void_p()
        check(lib.crychic_ctx_create(int(device_ordinal), C.byref(self.handle)))
        self.device = torch.device("cuda", int(device_ordinal))

    @property
    def device_name(self):
        return lib.crychic_ctx_device_name(self.handle).decode()

    def close(self):
        if self.handle:
            lib.crychic_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ssao:
    """Ssao.h:10-125.  Owns the view-normal map, the two half-res ambient maps, the random-vector map and the
    half-res edge workspace; ComputeSsao runs SSAO + blurCount x (H, V) blur on the caller's stream."""

    MaxBlurRadius = 5  # Ssao.h:24

    def __init__(self, ctx, width, height, randvec):
        self.ctx = ctx
        self.mRandomVectorMap = randvec
        self.OnResize(width, height)

    def OnResize(self, newWidth, newHeight):  # Ssao.cpp:164-183
        if newWidth % 2 or newHeight % 2:
            raise _lib.CrychicError(-1, "frame size must be even")
        self.mRenderTargetWidth, self.mRenderTargetHeight = newWidth, newHeight
        dev = self.ctx.device
        w2, h2 = newWidth // 2, newHeight // 2
        self.mNormalMap = torch.zeros((newHeight, newWidth, 4), device=dev, dtype=torch.float16)
        self.mNormalMap[..., 2] = 1.0  # clear (0,0,1,0), Ssao.cpp:317
        self.mAmbientMap0 = torch.full((h2, w2), -1, device=dev, dtype=torch.int16)  # R16_UNORM 1.0, Ssao.cpp:333
        self.mAmbientMap1 = torch.full((h2, w2), -1, device=dev, dtype=torch.int16)
        self.mEdge = torch.zeros((int(lib.crychic_edge_plane_bytes(newWidth, newHeight)),), device=dev, dtype=torch.uint8)

    def SsaoMapWidth(self):  # Ssao.cpp:22-25
        return self.mRenderTargetWidth // 2

    def SsaoMapHeight(self):  # Ssao.cpp:27-30
        return self.mRenderTargetHeight // 2

    @staticmethod
    def CalcGaussWeights(sigma):  # Ssao.cpp:37-68
        w = (C.c_float * 11)()
        n = check(lib.crychic_calc_gauss_weights(float(sigma), w, 11))
        return [w[i] for i in range(n)]

    def NormalMap(self):  # Ssao.cpp:70-73
        return self.mNormalMap

    def AmbientMap(self):  # Ssao.cpp:75-78
        return self.mAmbientMap0

    def ComputeSsao(self, depth, ssao_cb, blurCount, row0=0, rows=None):  # Ssao.cpp:185-229
        W, H = self.mRenderTargetWidth, self.mRenderTargetHeight
        rows = H // 2 - row0 if rows is None else rows
        check(lib.crychic_ssao_compute(self.ctx.handle, C.byref(ssao_cb), _ptr(self.mNormalMap), _ptr(depth),
                                       _ptr(self.mRandomVectorMap), _ptr(self.mAmbientMap0), _ptr(self.mAmbientMap1),
                                       _ptr(self.mEdge), W, H, int(blurCount), int(row0), int(rows),
                                       _stream(self.ctx.device)))

    def BlurAmbientMap(self, ssao_cb, horzBlur, row0=0, rows=None):  # Ssao.cpp:245-293
        W, H = self.mRenderTargetWidth, self.mRenderTargetHeight
        rows = H // 2 - row0 if rows is None else rows
        src, dst = (self.mAmbientMap0, self.mAmbientMap1) if horzBlur else (self.mAmbientMap1, self.mAmbientMap0)
        check(lib.crychic_ssao_blur(self.ctx.handle, C.byref(ssao_cb), _ptr(self.mEdge), _ptr(src), _ptr(dst), W, H,
                                    1 if horzBlur else 0, int(row0), int(rows), _stream(self.ctx.device)))


GBUFFER_FORMAT_NAMES = {"f32": ("f32", "f32", "f32"), "mixed": ("f32", "f16", "f16"), "f16": ("f16", "f16", "f16")}
_GBUFFER_DTYPES = {"f32": torch.float32, "f16": torch.float16}


def gbuffer_formats(formats):
    """The per-plane formats ("f32" | "f16" for G0, G1, G2) of a name -- "f32", "mixed" (G0 float4, G1 + G2 half4: 32 bytes per
    pixel) or "f16" (all three half4: 24 bytes, DXGI_FORMAT_R16G16B16A16_FLOAT) -- or of a sequence of three formats."""
    if isinstance(formats, str):
        formats = GBUFFER_FORMAT_NAMES.get(formats, (formats,))
    formats = tuple(formats) if formats is not None else ()
    if len(formats) != 3 or any(f not in _GBUFFER_DTYPES for f in formats):
        raise CrychicError(-3, "G-buffer formats %r: 'f32', 'mixed', 'f16' or three of 'f32' / 'f16'" % (formats,))
    return formats


def gbuffer_flags(planes):
    """The CRYCHIC_GBUFFER_G*_F16 bits of three G-buffer planes, from the tensors' dtypes."""
    flags = 0
    for k, g in enumerate(planes):
        if g.dtype == torch.float16:
            flags |= _lib.GBUFFER_G0_F16 << k
        elif g.dtype != torch.float32:
            raise CrychicError(-3, "G-buffer plane %d is %s: float32 or float16" % (k, g.dtype))
    return flags


class DeferredShading:
    """DeferredShading.h:4-45: owns the G-buffer planes (R32G32B32A32_FLOAT in the reference, CRYCHIC.cpp:56-58).  The reference
    allocates four; GBuffer3 carries no information (GBuffer.hlsl:29) and is not allocated here.  formats: each plane float4
    ("f32") or half4 ("f16"), see gbuffer_formats; a plane is allocated at its own size."""

    def __init__(self, ctx, width, height, formats=("f32", "f32", "f32")):
        self.ctx = ctx
        self.mFormats = gbuffer_formats(formats)
        self.OnResize(width, height)

    def OnResize(self, newWidth, newHeight):  # DeferredShading.cpp:79-93
        self.mWidth, self.mHeight = newWidth, newHeight
        self.mGBuffer = [torch.zeros((newHeight, newWidth, 4), device=self.ctx.device, dtype=_GBUFFER_DTYPES[f]) for f in self.mFormats]

    def Format(self, plane):
        return self.mFormats[plane]

    def Width(self):
        return self.mWidth

    def Height(self):
        return self.mHeight

    def Resource(self, index):  # DeferredShading.cpp:30-33
        return self.mGBuffer[index]


class ShadowMap:
    """ShadowMap.h:4-47: the cascade depth maps (D24 in uint32).  The reference allocates 12 x 12 slices of which
    4 cascades are valid (CRYCHIC.cpp:644)."""

    def __init__(self, ctx, width, height):
        if width != height:
            raise _lib.CrychicError(-1, "shadow maps are square")
        self.ctx = ctx
        self.mWidth, self.mHeight = width, height
        self.mShadowMap = torch.full((4, height, width), 0xFFFFFF, device=ctx.device, dtype=torch.int32)  # depth 1.0

    def Width(self):
        return self.mWidth

    def Height(self):
        return self.mHeight

    def Resource(self, index):
        return self.mShadowMap[index]


class Crychic:
    """Headless CRYCHIC (CRYCHIC.h:56-190): Draw() issues the hot part of CRYCHIC::Draw's deferred branch
    (CRYCHIC.cpp:220-221, 238-279) on this GPU's stream for the full-res rows [row0, row0 + rows)."""

    def __init__(self, ctx, width, height, randvec, cube, shadow_dim=4096, gbuffer_formats="f32"):
        self.ctx = ctx
        self.mClientWidth, self.mClientHeight = width, height
        self.mShadowMap = ShadowMap(ctx, shadow_dim, shadow_dim)
        self.mSsao = Ssao(ctx, width, height, randvec)
        self.mDeferred = DeferredShading(ctx, width, height, gbuffer_formats)
        self.mCubeMap = cube
        self.mCubeMapLevels = 1      # set_cube_map: > 1 = mCubeMap is a flat mip chain (CRYCHIC_LIGHT_CUBE_LEVELS), mCubeMapSize its level-0 face size
        self.mCubeMapSize = None
        self.mCubeMapGloss = False   # set_cube_map(gloss=True): the chain is prefiltered by roughness (CRYCHIC_LIGHT_CUBE_GLOSS)
        self.mCubeMapEnvBrdf = False     # set_cube_map(env_brdf=True): the environment BRDF table follows the environment tail (CRYCHIC_LIGHT_ENV_BRDF)
        self.mCubeMapAmbientSH = False   # set_cube_map(ambient_sh=True): the environment tail follows the cube map (CRYCHIC_LIGHT_AMBIENT_SH)
        self.mCubeMapParallax = False    # set_cube_map(parallax=True): the probe volume in the environment tail corrects the reflection lookup (CRYCHIC_LIGHT_CUBE_PARALLAX)
        self.mDepthStencilBuffer = torch.full((height, width), 0xFFFFFF, device=ctx.device, dtype=torch.int32)
        self.mBackBuffer = torch.zeros((height, width, 4), device=ctx.device, dtype=torch.uint8)
        self.mMainPassCB = PassConstants()
        self.mSsaoCB = SsaoConstants()
        self.blurCount = 3           # CRYCHIC.cpp:221
        self.numDirLights = 1        # NUM_DIR_LIGHTS of the deferred shader, Common.hlsl:6-8
        self.pcfSearchRadius = lib.crychic_pcf_search_radius(shadow_dim, 1)  # Common.hlsl:305 as written
        self.pcfLiteral = 1          # capture_environment: the `literal` of crychic_pcf_search_radius for the capture's own shadow map
        self.flags = 0
        self._probes = {}            # capture_environment: (dim, shadow_dim) -> the dim x dim probe renderer, kept across captures
        self._probe_chains = {}      # capture_environment(prefilter=True): (dim, levels) -> the scratch box chain
        self.mPointLights = None     # extension: torch uint8 tensor holding an array of Light structs (48 B each)
        self.mSpotLights = None      # extension: the same for the spot lights (the hot path's spot list)
        self.mSpotShadowMaps = None  # extension: (count, dim, dim) int32 D24 maps of the first spot lights (set_spot_shadows)
        self._spotHost = None        # host copy of the spot lights (the shadow transforms are built from it)
        self._spotShadow = None      # (SpotShadows descriptor, [transposed transform], [shadow pass constants], geometry)
        self.mPointShadowMaps = None  # extension: (count, 6, dim, dim) int32 D24 cube faces of the first point lights (set_point_shadows)
        self._pointHost = None       # host copy of the point lights (the face transforms are built from it)
        self._pointShadow = None     # (PointShadows descriptor, [face pass constants, 6 per light], geometry)
        self._desc = None
        self._followSun = None       # followSun, extension: None | True | SkyParams -- Draw() keeps a procedural sky bound whose sun is Lights[0]
        self._skyKey, self._skyChain = None, None    # what the sky in _skyChain, followSun's own chain, was rendered from
        self.skyRenders = 0          # launches of crychic_render_sky this object has issued (render_sky and followSun)
        # The switches of the passes behind the lighting pass (the properties below): Draw() looks at _post alone, so a frame with none
        # of them set pays one test however many passes there are.
        self._post = False
        self._antiAliasing = None    # antiAliasing, extension: None | True | AAParams -- Draw() of a whole frame runs crychic_antialias into mBackBufferAA
        self.mBackBufferAA = None    # the anti-aliased frame, allocated by the first antialias() that needs it
        self._fog = None             # fog, extension: None | True | FogParams -- Draw() of a whole frame runs crychic_fog in place on mBackBuffer
        self._ssr = None             # ssr, extension: None | True | SsrParams -- Draw() of a whole frame runs crychic_ssr into mBackBufferSSR, in front of the fog
        self.mBackBufferSSR = None   # the frame behind the screen-space reflections, allocated by the first screen_space_reflections() that needs it
        self._ssrGloss = None        # ssrGloss, extension: None | True | SsrGlossParams -- with ssr set, Draw() runs crychic_ssr_pyramid and crychic_ssr_glossy in place of crychic_ssr
        self.mSsrPyramid = None      # the lit frame's pyramid: crychic_ssr_pyramid_bytes of the frame at the most levels, with the first ssr_pyramid()
        self._depthOfField = None    # depthOfField, extension: None | True | DofParams -- Draw() of a whole frame runs crychic_dof into mBackBufferDoF
        self.mBackBufferDoF = None   # the frame behind the depth-of-field pass, allocated by the first depth_of_field() that needs it
        self._bloom = None           # bloom, extension: None | True | BloomParams -- Draw() of a whole frame runs crychic_bloom into mBackBufferBloom
        self.mBackBufferBloom = None  # the frame behind the bloom pass, allocated by the first apply_bloom() that needs it
        self.mBloomWorkspace = None  # the pass's pyramid: crychic_bloom_workspace_bytes of the frame at the most levels, with the first apply_bloom()
        self._temporalAA = None      # temporalAA, extension: None | True | TaaParams -- Draw() of a whole frame runs crychic_taa into mBackBufferTAA
        self.mBackBufferTAA = None   # the resolved frame, allocated by the first temporal_aa() that needs it
        self.mTaaHistory = None      # [history read by the next call, history it writes]: (H, W, 4) int16 planes of 8.8 fixed point, swapped after each call
        self._taaReset = True        # the next Draw() with temporalAA set is a RESET frame: the first, or the first after the switch was turned on
        self._taaViewProj = [None, None]     # set_frame_view_proj: the unjittered ViewProj of this frame and of the previous one
        self._frameJitter = (0.0, 0.0)       # set_frame_view_proj: the jitter the frame's constants were built with
        self._temporalUpscale = None  # temporalUpscale, extension: None | (Wo, Ho) | (Wo, Ho, TaaUpscaleParams) -- Draw() of a whole frame runs crychic_taa_upscale into mBackBufferUpscaled
        self.mBackBufferUpscaled = None      # the resolved (Ho, Wo, 4) frame of the display size, allocated by the first temporal_upscale() that needs it
        self.mTaaUpscaleHistory = None       # as mTaaHistory, of the display size
        self._taaUpscaleReset = True         # as _taaReset, for temporalUpscale
        self._sharpening = None      # sharpening, extension: None | True | SharpenParams -- Draw() of a whole frame runs crychic_sharpen into mBackBufferSharp, behind the temporal stage
        self.mBackBufferSharp = None  # the sharpened frame, allocated by the first sharpen_frame() that needs it
        self._motionBlur = None      # motionBlur, extension: None | True | MotionBlurParams -- Draw() of a whole frame runs crychic_motion_blur into mBackBufferMB
        self.mBackBufferMB = None    # the frame behind the motion blur, allocated by the first motion_blur() that needs it
        self.mMotionBlurWorkspace = None     # the velocity and tile planes: crychic_motion_blur_workspace_bytes of the frame, with the first motion_blur()
        self._colourGrade = None     # colourGrade, extension: None | GradeParams | (N, N, N, 4) uint8 array | path of a .cube file -- Draw() of a whole frame runs crychic_grade into mBackBufferGrade
        self.mBackBufferGrade = None  # the graded frame, allocated by the first colour_grade() that needs it
        self.mGradeLut = None        # the table colourGrade was given, built or loaded and uploaded once by the assignment: an (N, N, N, 4) uint8 device tensor, [blue][green][red]
        self.mDecals, self.mDecalCount = None, 0                             # set_decals, extension: the device array of Decal structs
        self._decalTextures, self._decalTextureCount, self._decalKeep = None, 0, []     # the host texture table and the chains it points into

    def _post_switch(name):          # noqa: N805 -- a class-body helper: the property of one switch
        def get(self):
            return getattr(self, name)

        def put(self, value):
            if name == "_temporalAA" and value and not self._temporalAA:
                self._taaReset = True            # turned on: whatever the history planes hold is stale
            if name == "_temporalUpscale" and value and not self._temporalUpscale:
                self._taaUpscaleReset = True
            setattr(self, name, value)
            self._update_post()
        return property(get, put)

    def _update_post(self):
        self._post = bool(self._fog or self._antiAliasing or self._depthOfField or self._bloom or self._temporalAA or self._motionBlur or self._ssr or self._ssrGloss
                          or self._temporalUpscale or self._colourGrade is not None or self._sharpening)

    antiAliasing = _post_switch("_antiAliasing")
    fog = _post_switch("_fog")
    ssr = _post_switch("_ssr")
    ssrGloss = _post_switch("_ssrGloss")
    depthOfField = _post_switch("_depthOfField")
    bloom = _post_switch("_bloom")
    temporalAA = _post_switch("_temporalAA")
    motionBlur = _post_switch("_motionBlur")
    temporalUpscale = _post_switch("_temporalUpscale")
    sharpening = _post_switch("_sharpening")

    @property
    def colourGrade(self):
        return self._colourGrade

    @colourGrade.setter
    def colourGrade(self, value):
        """None | a GradeParams (crychic_grade_build_lut at GRADE_MAX_N) | an (N, N, N, 4) uint8 array or tensor indexed [blue][green][red]
        | the path of a .cube file (crychic_load_cube_lut): the table is built or loaded and uploaded here, once."""
        self.mGradeLut = None if value is None else self.grade_lut(value)
        self._colourGrade = value
        self._update_post()

    def grade_lut(self, value):
        """The (N, N, N, 4) uint8 device tensor of a table given as colourGrade takes it."""
        if isinstance(value, GradeParams):
            N = _lib.GRADE_MAX_N
            buf = (C.c_uint8 * (4 * N ** 3))()
            check(lib.crychic_grade_build_lut(C.byref(value), N, buf, len(buf)))
        elif isinstance(value, (str, bytes)) or hasattr(value, "__fspath__"):
            import os
            path = os.fsencode(value)
            n = C.c_uint32()
            buf = (C.c_uint8 * (4 * _lib.GRADE_MAX_N ** 3))()
            rc = lib.crychic_load_cube_lut(path, buf, len(buf), C.byref(n))
            if rc < 0:
                raise CrychicError(rc, "crychic_load_cube_lut refuses %r" % (value,))
            N = int(n.value)
        else:
            t = value if isinstance(value, torch.Tensor) else torch.tensor(value)      # a copy: the caller's array may be read-only
            if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 4 or not (t.shape[0] == t.shape[1] == t.shape[2]) \
                    or not 2 <= t.shape[0] <= _lib.GRADE_MAX_N:
                raise CrychicError(-1, "a colour grade table is an (N, N, N, 4) uint8 array, 2 <= N <= %d" % _lib.GRADE_MAX_N)
            return t.to(self.ctx.device).contiguous().clone()
        return torch.frombuffer(buf, dtype=torch.uint8, count=4 * N ** 3).reshape(N, N, N, 4).to(self.ctx.device)
    del _post_switch

    def set_gbuffer_formats(self, formats):
        """Re-allocates the G-buffer in the given formats (gbuffer_formats: "f32", "mixed", "f16" or three per-plane formats); its
        contents are lost, as on a resize.  The producers and the lighting pass take each plane's format from its tensor."""
        self.mDeferred = DeferredShading(self.ctx, self.mClientWidth, self.mClientHeight, formats)
        self._desc = None

    def load_scene(self, planes):
        """Install externally produced input planes (scene.make_scene) in place of the producer passes.  A G-buffer plane arrives in
        float32 and is converted to its format here (torch's float32 -> float16: round to nearest even, subnormals kept, overflow to
        infinity -- the producers' conversion); planes already in the format are installed as they are."""
        self.mDepthStencilBuffer = planes["depth"]
        self.mSsao.mNormalMap = planes["normal"]
        self.mDeferred.mGBuffer = [planes["g%d" % k].to(_GBUFFER_DTYPES[self.mDeferred.mFormats[k]]) for k in range(3)]
        self.mShadowMap.mShadowMap = planes["shadow"]
        self.mCubeMap = planes["cube"]
        self.mCubeMapLevels, self.mCubeMapSize, self.mCubeMapGloss, self.mCubeMapAmbientSH, self.mCubeMapEnvBrdf = 1, None, False, False, False
        self.mCubeMapParallax = False
        self.mSsao.mRandomVectorMap = planes["randvec"]
        self.mMainPassCB = planes["consts"].pass_cb
        self.mSsaoCB = planes["consts"].ssao_cb
        self._desc = None

    def frame_desc(self, row0=0, rows=None):
        W, H = self.mClientWidth, self.mClientHeight
        f = FrameDesc()
        f.W, f.H = W, H
        f.blurCount, f.numDirLights = int(self.blurCount), int(self.numDirLights)
        f.pcfSearchRadius, f.flags = float(self.pcfSearchRadius), int(self.flags) | ((int(self.mCubeMapLevels) & 15) << 16 if self.mCubeMapLevels > 1 else 0)
        if self.mCubeMapGloss:
            f.flags |= _lib.LIGHT_CUBE_GLOSS
        if self.mCubeMapAmbientSH:
            f.flags |= _lib.LIGHT_AMBIENT_SH
        if self.mCubeMapEnvBrdf:
            f.flags |= _lib.LIGHT_ENV_BRDF
        if self.mCubeMapParallax:
            f.flags |= _lib.LIGHT_CUBE_PARALLAX
        f.flags = (f.flags & ~_lib.GBUFFER_F16_MASK) | gbuffer_flags(self.mDeferred.mGBuffer)      # each plane's format: its tensor's dtype
        f.row0, f.rows = int(row0), int(H - row0 if rows is None else rows)
        f.normal_dev = self.mSsao.mNormalMap.data_ptr()
        f.depth_dev = self.mDepthStencilBuffer.data_ptr()
        f.randvec_dev = self.mSsao.mRandomVectorMap.data_ptr()
        f.g0_dev, f.g1_dev, f.g2_dev = (g.data_ptr() for g in self.mDeferred.mGBuffer)
        for i in range(4):
            f.shadow_dev[i] = self.mShadowMap.mShadowMap[i].data_ptr()
        f.shadowDim = self.mShadowMap.Width()
        f.cube_dev, f.cubeDim = self.mCubeMap.data_ptr(), int(self.mCubeMapSize or self.mCubeMap.shape[1])
        f.ambient0_dev = self.mSsao.mAmbientMap0.data_ptr()
        f.ambient1_dev = self.mSsao.mAmbientMap1.data_ptr()
        f.edge_dev = self.mSsao.mEdge.data_ptr()
        f.out_rgba8_dev = self.mBackBuffer.data_ptr()
        if self.mPointLights is not None:
            f.point_lights_dev = self.mPointLights.data_ptr()
            f.numPointLights = self.mPointLights.numel() // 48
        return f

    def Draw(self, row0=0, rows=None, shared=None):  # CRYCHIC.cpp:172-306 (hot part)
        """shared = (communicator handle, bounds array or None, parts): the _shared entry -- the strip AND its exchange,
        the lighting pass in `parts` row ranges that travel while the next is lit (sharding.StripExchange.draw).
        With a switch of the passes behind the lighting pass set (extensions; True, or the pass's parameter struct): a whole frame,
        then the set passes in the order
            lighting -> ssr (with ssrGloss: the lit frame's pyramid and the glossy variant) -> fog (in place on the frame it is handed) -> temporalAA -> sharpening -> depthOfField -> motionBlur -> bloom -> colourGrade -> antiAliasing,
        each but the fog from the buffer of the nearest set stage in front of it that writes one of its own (mBackBuffer if there is
        none) into its own mBackBuffer*; final_frame() is the last one.  The temporal pass and the motion blur take the matrices of
        set_frame_view_proj (never called: a still camera); the first frame after temporalAA was turned on is a RESET frame.  A strip
        or a shared draw then raises CrychicError: these passes are not sharded.
        temporalUpscale = (Wo, Ho) or (Wo, Ho, TaaUpscaleParams) puts crychic_taa_upscale at the temporal pass's place: the frame of the
        client size, rendered with the jitter handed to set_frame_view_proj, is accumulated into a history of Wo x Ho texels, and the
        sharpening, the bloom, the colour grade and the anti-aliasing behind it run at that size.  Together with temporalAA, depthOfField or motionBlur it raises
        CrychicError before anything is issued (the last two read a depth plane of the frame's size).
        followSun (extension; True or a SkyParams): in front of all that, the procedural sky is kept bound whose sun is where Lights[0]
        shines from (render_sky), re-rendered only when that direction or the parameters changed; strips and shared draws included."""
        if self._followSun is not None:
            self._follow_sun()
        if self._post:
            return self._draw_post_chain(row0, rows, shared)
        return self._draw_lighting(row0, rows, shared)

    def _draw_lighting(self, row0, rows, shared):
        """The lighting frame: all of Draw() while no switch is set."""
        # The descriptor only changes when a plane is re-allocated or a knob is turned: keep it across frames so the
        # per-frame host cost is one FFI call (matters once a strip takes tens of microseconds on 8 GPUs).  The key holds
        # every device pointer and size frame_desc() reads, so replacing any plane object invalidates the cached descriptor.
        ssao, sm = self.mSsao, self.mShadowMap.mShadowMap
        g0, g1, g2 = self.mDeferred.mGBuffer
        key = (row0, rows, self.mBackBuffer.data_ptr(), ssao.mAmbientMap0.data_ptr(), ssao.mAmbientMap1.data_ptr(), ssao.mEdge.data_ptr(),
               ssao.mNormalMap.data_ptr(), ssao.mRandomVectorMap.data_ptr(), self.mDepthStencilBuffer.data_ptr(),
               g0.data_ptr(), g1.data_ptr(), g2.data_ptr(), g0.dtype, g1.dtype, g2.dtype,
               sm.data_ptr(), int(sm.shape[-1]), self.mCubeMap.data_ptr(), int(self.mCubeMapSize or self.mCubeMap.shape[1]), int(self.mCubeMapLevels),
               self.mCubeMapGloss, self.mCubeMapAmbientSH, self.mCubeMapEnvBrdf, self.mCubeMapParallax, self.blurCount, self.numDirLights, self.pcfSearchRadius, self.flags,
               0 if self.mPointLights is None else self.mPointLights.data_ptr(),
               0 if self.mSpotLights is None else self.mSpotLights.data_ptr())
        if self._desc is None:
            self._desc = {}
        f = self._desc.get(key)          # the descriptor's reference, as the entries take it
        if f is None:
            if len(self._desc) > 16:
                self._desc.clear()
            f = self._desc[key] = C.byref(self.frame_desc(row0, rows))
        # One entry, frame, strip or shared: the local lights' lists and shadow descriptors (extensions) are None where there are
        # none, which the library serves as the narrower entries do, bit for bit (include/crychic_hip.h).
        spots, n = (None, 0) if self.mSpotLights is None else (_ptr(self.mSpotLights), self.mSpotLights.numel() // 48)
        pcb, desc, pdesc = self.mMainPassCB, None, None
        if self._spotShadow is not None:
            d, T, cbs, geo = self._spotShadow
            desc = C.byref(d)
            pcb = PassConstants.from_buffer_copy(self.mMainPassCB)      # mMainPassCB with the spot transforms in slots 4..11
            for k, t in enumerate(T):
                pcb.ShadowTransforms[4 + k][:] = t
            if geo is not None:
                self.DrawSpotShadowMaps()
        if self._pointShadow is not None:
            pd, _, pgeo = self._pointShadow
            pdesc = C.byref(pd)
            if pgeo is not None:
                self.DrawPointShadowMaps()
        if shared is not None:
            check(lib.crychic_draw_hot_path_shared_point_shadows(shared[0], C.byref(self.mSsaoCB), C.byref(pcb), f, shared[1],
                                                                 int(shared[2]), spots, n, desc, pdesc, _stream(self.ctx.device)))
        else:
            check(lib.crychic_draw_hot_path_point_shadows(self.ctx.handle, C.byref(self.mSsaoCB), C.byref(pcb), f, spots, n, desc,
                                                          pdesc, _stream(self.ctx.device)))

    def _draw_post_chain(self, row0, rows, shared):
        """Draw() with a switch set: the lighting frame, then one walk along the chain with the frame each stage reads."""
        if shared is not None or row0 != 0 or (rows is not None and rows != self.mClientHeight):
            what = next(s for s in ("bloom", "motionBlur", "depthOfField", "temporalAA", "fog", "antiAliasing", "ssr", "temporalUpscale", "colourGrade", "ssrGloss", "sharpening")
                        if (getattr(self, s) is not None if s == "colourGrade" else getattr(self, s)))
            raise CrychicError(-1, "%s is set: Draw() takes the whole frame on one GPU (the pass is not sharded and does not run behind the "
                               "exchange)" % what)
        if self._ssrGloss and not self._ssr:
            raise CrychicError(-1, "ssrGloss is set and ssr is not: the glossy lookup is a variant of the screen-space reflections")
        if self._temporalUpscale:
            for other in ("temporalAA", "depthOfField", "motionBlur"):
                if getattr(self, other):
                    raise CrychicError(-1, "temporalUpscale and %s are both set: %s" % (other, "one temporal pass resolves a frame" if other == "temporalAA"
                                                                                        else "the pass reads a depth plane of the frame's size, and the frame behind the upsampling has the display's"))
            up = tuple(self._temporalUpscale)
            if len(up) not in (2, 3) or (len(up) == 3 and not isinstance(up[2], TaaUpscaleParams)):
                raise CrychicError(-1, "temporalUpscale takes (Wo, Ho) or (Wo, Ho, TaaUpscaleParams)")
        self._draw_lighting(0, None, None)

        def params(switch, kind):               # a switch holds True or the pass's parameters
            return switch if isinstance(switch, kind) else None
        frame = self.mBackBuffer
        if self._ssr:
            if self._ssrGloss:
                gloss = params(self._ssrGloss, SsrGlossParams) or SsrGlossParams.default()
                self.ssr_pyramid(src=frame, levels=gloss.levels)
                frame = self.screen_space_reflections(src=frame, params=params(self._ssr, SsrParams), gloss=gloss)
            else:
                frame = self.screen_space_reflections(src=frame, params=params(self._ssr, SsrParams))
        if self._fog:
            self.apply_fog(src=frame, params=params(self._fog, FogParams))
        cur, prev = self._taaViewProj           # of the temporal pass and the motion blur
        if cur is None:                         # set_frame_view_proj was never called: a still camera whose constants are not jittered
            cur = prev = tuple(self.mMainPassCB.ViewProj)
        elif prev is None:                      # no previous frame
            prev = cur
        if self._temporalAA:
            frame = self.temporal_aa(cur, prev, src=frame, reset=self._taaReset, params=params(self._temporalAA, TaaParams))
            self._taaReset = False
        if self._temporalUpscale:
            frame = self.temporal_upscale(cur, prev, self._frameJitter, up[:2], src=frame, reset=self._taaUpscaleReset, params=up[2] if len(up) == 3 else None)
            self._taaUpscaleReset = False
        if self._sharpening:                    # directly behind the temporal stage, at its place when there is none
            frame = self.sharpen_frame(src=frame, params=params(self._sharpening, SharpenParams))
        if self._depthOfField:
            frame = self.depth_of_field(src=frame, params=params(self._depthOfField, DofParams))
        if self._motionBlur:
            frame = self.motion_blur(cur, prev, src=frame, params=params(self._motionBlur, MotionBlurParams))
        if self._bloom:
            frame = self.apply_bloom(src=frame, params=params(self._bloom, BloomParams))
        if self._colourGrade is not None:
            frame = self.colour_grade(src=frame)
        if self._antiAliasing:
            self.antialias(src=frame, params=params(self._antiAliasing, AAParams))

    def final_frame(self):
        """The tensor a Draw() with the switches as they are leaves the finished frame in: the last set stage's buffer."""
        for switch, name in ((self._antiAliasing, "mBackBufferAA"), (self._colourGrade is not None, "mBackBufferGrade"), (self._bloom, "mBackBufferBloom"), (self._motionBlur, "mBackBufferMB"),
                             (self._depthOfField, "mBackBufferDoF"), (self._sharpening, "mBackBufferSharp"), (self._temporalAA, "mBackBufferTAA"), (self._temporalUpscale, "mBackBufferUpscaled")):
            if switch:
                return getattr(self, name)
        return self.mBackBufferSSR if self._ssr else self.mBackBuffer

    def _pass_frames(self, who, buffer, src, out, any_shape=False):
        """(src, out, H, W) of the pass method `who`: src defaults to mBackBuffer, out to the attribute `buffer` -- allocated, or
        re-allocated to src's shape and device, on first use -- or with buffer None to src (in place); both checked."""
        src = self.mBackBuffer if src is None else src
        if out is None and buffer is None:
            out = src
        elif out is None:
            out = getattr(self, buffer)
            if out is None or out.shape != src.shape or out.device != src.device:
                out = torch.zeros_like(src)
                setattr(self, buffer, out)
        H, W = int(src.shape[0]), int(src.shape[1])
        if src.dtype != torch.uint8 or out.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 4 or out.shape != src.shape \
                or not src.is_contiguous() or not out.is_contiguous() or not (any_shape or (H, W) == (self.mClientHeight, self.mClientWidth)):
            raise CrychicError(-1, "%s takes contiguous (H, W, 4) uint8 tensors of %s" % (who, "one shape" if any_shape else "the frame's size"))
        return src, out, H, W

    def motion_blur(self, cur_view_proj, prev_view_proj, src=None, out=None, row0=0, rows=None, params=None):
        """crychic_motion_blur on the context's stream: rows [row0, row0 + rows) of `out` (default: mBackBufferMB, allocated on first
        use) from `src` (default: mBackBuffer), both (H, W, 4) uint8 tensors of the frame's size, with this frame's depth plane and
        pass constants and the two UNJITTERED view-projections (16 floats each, stored transposed).  The velocity and tile planes go
        through mMotionBlurWorkspace, allocated on first use: the velocity launch always covers the whole frame, the gather the row
        range.  params: a MotionBlurParams, None = the defaults.  `src` and `out` must not overlap.  Returns `out`."""
        src, out, H, W = self._pass_frames("motion_blur", "mBackBufferMB", src, out)
        need = int(lib.crychic_motion_blur_workspace_bytes(W, H))
        if self.mMotionBlurWorkspace is None or self.mMotionBlurWorkspace.numel() != need or self.mMotionBlurWorkspace.device != src.device:
            self.mMotionBlurWorkspace = torch.zeros((need,), dtype=torch.uint8, device=src.device)
        p = C.byref(params) if params is not None else None
        cur, prev = (C.c_float * 16)(*cur_view_proj), (C.c_float * 16)(*prev_view_proj)
        ws, stream = _ptr(self.mMotionBlurWorkspace), _stream(self.ctx.device)
        if row0 == 0 and (rows is None or rows == H):
            check(lib.crychic_motion_blur(self.ctx.handle, C.byref(self.mMainPassCB), cur, prev, self.mDepthStencilBuffer.data_ptr(), _ptr(src), _ptr(out),
                                          W, H, p, ws, need, stream))
        else:
            check(lib.crychic_motion_blur_velocity(self.ctx.handle, C.byref(self.mMainPassCB), cur, prev, self.mDepthStencilBuffer.data_ptr(), W, H, p, ws,
                                                   need, stream))
            check(lib.crychic_motion_blur_gather(self.ctx.handle, _ptr(src), _ptr(out), W, H, int(row0), int(H - row0 if rows is None else rows), p, ws,
                                                 need, stream))
        return out

    def set_frame_view_proj(self, view_proj, jitter=(0.0, 0.0)):
        """The UNJITTERED view-projection of the frame about to be drawn (16 floats, stored transposed like the pass constants'
        ViewProj): what was current becomes the previous frame's.  Draw() with temporalAA set hands both to crychic_taa.  jitter: the
        (jx, jy) the frame's constants were built with, which Draw() with temporalUpscale set hands to crychic_taa_upscale."""
        m = tuple(float(v) for v in view_proj)
        j = tuple(float(v) for v in jitter)
        if len(m) != 16 or len(j) != 2:
            raise CrychicError(-1, "set_frame_view_proj takes 16 floats and a jitter of 2")
        self._taaViewProj = [m, self._taaViewProj[0]]
        self._frameJitter = j

    def temporal_upscale(self, cur_view_proj, prev_view_proj, jitter, display_size, src=None, out=None, reset=False, row0=0, rows=None, params=None):
        """crychic_taa_upscale on the context's stream: rows [row0, row0 + rows) of `out` (default: mBackBufferUpscaled, allocated on
        first use), an (Ho, Wo, 4) uint8 tensor of display_size = (Wo, Ho), from `src` (default: mBackBuffer), an (H, W, 4) uint8 tensor
        of the frame's size, with this frame's depth plane and (jittered) pass constants, the two UNJITTERED view-projections (16
        floats each, stored transposed) and the frame's jitter (jx, jy).  The two history planes mTaaUpscaleHistory, of the display
        size, are this object's and behave as mTaaHistory does in temporal_aa.  params: a TaaUpscaleParams, None = the defaults.
        Returns `out`."""
        src = self.mBackBuffer if src is None else src
        Wo, Ho = int(display_size[0]), int(display_size[1])
        if out is None:
            out = self.mBackBufferUpscaled
            if out is None or out.shape != (Ho, Wo, 4) or out.device != src.device:
                out = self.mBackBufferUpscaled = torch.zeros((Ho, Wo, 4), dtype=torch.uint8, device=src.device)
        H, W = self.mClientHeight, self.mClientWidth
        if src.dtype != torch.uint8 or out.dtype != torch.uint8 or tuple(src.shape) != (H, W, 4) or tuple(out.shape) != (Ho, Wo, 4) \
                or not src.is_contiguous() or not out.is_contiguous():
            raise CrychicError(-1, "temporal_upscale takes a contiguous (H, W, 4) uint8 tensor of the frame's size and one of the display's")
        hist = self.mTaaUpscaleHistory
        if hist is None or tuple(hist[0].shape) != (Ho, Wo, 4) or hist[0].device != src.device:
            self.mTaaUpscaleHistory = [torch.zeros((Ho, Wo, 4), dtype=torch.int16, device=src.device) for _ in range(2)]
            reset = True
        p = TaaUpscaleParams.default() if params is None else TaaUpscaleParams.from_buffer_copy(params)
        if reset:
            p.flags |= _lib.TAA_RESET
        cur, prev = (C.c_float * 16)(*cur_view_proj), (C.c_float * 16)(*prev_view_proj)
        hin, hout = self.mTaaUpscaleHistory
        check(lib.crychic_taa_upscale(self.ctx.handle, C.byref(self.mMainPassCB), cur, prev, float(jitter[0]), float(jitter[1]),
                                      self.mDepthStencilBuffer.data_ptr(), _ptr(src), W, H, None if p.flags & _lib.TAA_RESET else _ptr(hin), _ptr(hout),
                                      _ptr(out), Wo, Ho, int(row0), int(Ho - row0 if rows is None else rows), C.byref(p), _stream(self.ctx.device)))
        self.mTaaUpscaleHistory = [hout, hin]
        return out

    def temporal_aa(self, cur_view_proj, prev_view_proj, src=None, out=None, reset=False, row0=0, rows=None, params=None):
        """crychic_taa on the context's stream: rows [row0, row0 + rows) of `out` (default: mBackBufferTAA, allocated on first use) from
        `src` (default: mBackBuffer), both (H, W, 4) uint8 tensors of the frame's size, with this frame's depth plane and (jittered)
        pass constants and the two UNJITTERED view-projections (16 floats each, stored transposed).  The two history planes
        mTaaHistory are this object's: allocated on first use (which makes the call a RESET call, as does reset=True or a RESET flag
        in params), read from [0], written to [1] and swapped after the call, so that mTaaHistory[0] is the history just written.
        params: a TaaParams, None = the defaults.  `src` and `out` must not overlap.  Returns `out`."""
        src, out, H, W = self._pass_frames("temporal_aa", "mBackBufferTAA", src, out)
        if self.mTaaHistory is None or self.mTaaHistory[0].shape != src.shape or self.mTaaHistory[0].device != src.device:
            self.mTaaHistory = [torch.zeros((H, W, 4), dtype=torch.int16, device=src.device) for _ in range(2)]
            reset = True
        p = TaaParams.default() if params is None else TaaParams.from_buffer_copy(params)
        if reset:
            p.flags |= _lib.TAA_RESET
        cur, prev = (C.c_float * 16)(*cur_view_proj), (C.c_float * 16)(*prev_view_proj)
        hin, hout = self.mTaaHistory
        check(lib.crychic_taa(self.ctx.handle, C.byref(self.mMainPassCB), cur, prev, self.mDepthStencilBuffer.data_ptr(), _ptr(src),
                              None if p.flags & _lib.TAA_RESET else _ptr(hin), _ptr(hout), _ptr(out), W, H, int(row0),
                              int(H - row0 if rows is None else rows), C.byref(p), _stream(self.ctx.device)))
        self.mTaaHistory = [hout, hin]
        return out

    def apply_bloom(self, src=None, out=None, params=None):
        """crychic_bloom on the context's stream: the whole frame `out` (default: mBackBufferBloom, allocated on first use) from `src`
        (default: mBackBuffer), both (H, W, 4) uint8 tensors of one shape (the frame's, or the display's behind temporalUpscale); `out`
        may be `src` itself (in place) and must not overlap it otherwise.  params: a BloomParams, None = the defaults.  The pyramid goes through mBloomWorkspace, allocated on
        first use for the frame's size at BLOOM_MAX_LEVELS levels; afterwards its level k holds U_k.  Returns `out`."""
        src, out, H, W = self._pass_frames("apply_bloom", "mBackBufferBloom", src, out, any_shape=True)
        need = int(lib.crychic_bloom_workspace_bytes(W, H, _lib.BLOOM_MAX_LEVELS))
        if self.mBloomWorkspace is None or self.mBloomWorkspace.numel() != need or self.mBloomWorkspace.device != src.device:
            self.mBloomWorkspace = torch.zeros((need,), dtype=torch.uint8, device=src.device)
        check(lib.crychic_bloom(self.ctx.handle, _ptr(src), _ptr(out), W, H, None if params is None else C.byref(params),
                                _ptr(self.mBloomWorkspace), need, _stream(self.ctx.device)))
        return out

    def colour_grade(self, src=None, out=None, lut=None, row0=0, rows=None):
        """crychic_grade on the context's stream: rows [row0, row0 + rows) of `out` (default: mBackBufferGrade, allocated on first use)
        from `src` (default: mBackBuffer), both (H, W, 4) uint8 tensors of one shape (the frame's, or the display's behind
        temporalUpscale), through the table `lut` (default: mGradeLut, what colourGrade was given; otherwise anything colourGrade
        takes, uploaded for this call).  `out` may be `src` itself (in place) and must not overlap it otherwise.  Returns `out`."""
        src, out, H, W = self._pass_frames("colour_grade", "mBackBufferGrade", src, out, any_shape=True)
        table = self.mGradeLut if lut is None else self.grade_lut(lut)
        if table is None:
            raise CrychicError(-1, "colour_grade needs a table: set colourGrade or pass lut")
        check(lib.crychic_grade(self.ctx.handle, _ptr(src), _ptr(out), W, H, int(row0), int(H - row0 if rows is None else rows), _ptr(table),
                                int(table.shape[0]), _stream(self.ctx.device)))
        return out

    def sharpen_frame(self, src=None, out=None, row0=0, rows=None, params=None):
        """crychic_sharpen on the context's stream: rows [row0, row0 + rows) of `out` (default: mBackBufferSharp, allocated on first use)
        from `src` (default: mBackBuffer), both (H, W, 4) uint8 tensors of one shape (the frame's, or the display's behind
        temporalUpscale).  params: a SharpenParams, None = the defaults.  `src` and `out` must not overlap.  Returns `out`."""
        src, out, H, W = self._pass_frames("sharpen_frame", "mBackBufferSharp", src, out, any_shape=True)
        check(lib.crychic_sharpen(self.ctx.handle, _ptr(src), _ptr(out), W, H, int(row0), int(H - row0 if rows is None else rows),
                                  C.byref(params) if params is not None else None, _stream(self.ctx.device)))
        return out

    def depth_of_field(self, src=None, out=None, row0=0, rows=None, params=None):
        """crychic_dof on the context's stream: rows [row0, row0 + rows) of `out` (default: mBackBufferDoF, allocated on first use)
        from `src` (default: mBackBuffer), both (H, W, 4) uint8 tensors of the frame's size, with this frame's depth plane and pass
        constants; params: a DofParams, None = the defaults.  The pass reads rows [row0 - R, row0 + rows + R) of `src` and of the
        depth plane and writes no other byte of `out`; `src` and `out` must not overlap.  Returns `out`."""
        src, out, H, W = self._pass_frames("depth_of_field", "mBackBufferDoF", src, out)
        check(lib.crychic_dof(self.ctx.handle, C.byref(self.mMainPassCB), self.mDepthStencilBuffer.data_ptr(), _ptr(src), _ptr(out), W, H,
                              int(row0), int(H - row0 if rows is None else rows), None if params is None else C.byref(params),
                              _stream(self.ctx.device)))
        return out

    def ssr_pyramid(self, src=None, levels=None):
        """crychic_ssr_pyramid on the context's stream: levels 1 .. n_eff of the pyramid of `src` (default: mBackBuffer; an (H, W, 4)
        uint8 tensor of the frame's size) into mSsrPyramid, allocated on first use for the frame's size at SSR_GLOSS_MAX_LEVELS levels;
        levels: 1 .. SSR_GLOSS_MAX_LEVELS, the frame counted, None = the default of SsrGlossParams.  Returns mSsrPyramid."""
        src, _, H, W = self._pass_frames("ssr_pyramid", None, src, None)
        levels = SsrGlossParams.default().levels if levels is None else int(levels)
        need = int(lib.crychic_ssr_pyramid_bytes(W, H, _lib.SSR_GLOSS_MAX_LEVELS))
        if self.mSsrPyramid is None or self.mSsrPyramid.numel() != max(need, 16) or self.mSsrPyramid.device != src.device:
            self.mSsrPyramid = torch.zeros((max(need, 16),), dtype=torch.uint8, device=src.device)
        check(lib.crychic_ssr_pyramid(self.ctx.handle, _ptr(src), W, H, levels, _ptr(self.mSsrPyramid), self.mSsrPyramid.numel(),
                                      _stream(self.ctx.device)))
        return self.mSsrPyramid

    def screen_space_reflections(self, src=None, out=None, row0=0, rows=None, params=None, gloss=None):
        """crychic_ssr on the context's stream: rows [row0, row0 + rows) of `out` (default: mBackBufferSSR, allocated on first use) from
        `src` (default: mBackBuffer), both (H, W, 4) uint8 tensors of the frame's size, with this frame's G-buffer in its planes'
        formats, depth plane and pass constants; params: an SsrParams, None = the defaults.  The pass reads any row of `src` and of the
        depth plane and writes no other byte of `out`; `src` and `out` must not overlap.  Returns `out`.
        gloss: None, or True or an SsrGlossParams for crychic_ssr_glossy in its place, which reads the hit colour from mSsrPyramid:
        what ssr_pyramid(src, levels=gloss.levels) left there, the caller's to issue first."""
        src, out, H, W = self._pass_frames("screen_space_reflections", "mBackBufferSSR", src, out)
        g = self.mDeferred.mGBuffer
        if gloss is not None:
            if self.mSsrPyramid is None:
                raise CrychicError(-1, "screen_space_reflections(gloss=...) reads mSsrPyramid: call ssr_pyramid() first")
            gp = gloss if isinstance(gloss, SsrGlossParams) else None
            check(lib.crychic_ssr_glossy(self.ctx.handle, C.byref(self.mMainPassCB), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                                         self.mDepthStencilBuffer.data_ptr(), _ptr(src), _ptr(self.mSsrPyramid), self.mSsrPyramid.numel(), _ptr(out), W,
                                         H, int(row0), int(H - row0 if rows is None else rows), gbuffer_flags(g),
                                         None if params is None else C.byref(params), None if gp is None else C.byref(gp), _stream(self.ctx.device)))
            return out
        check(lib.crychic_ssr(self.ctx.handle, C.byref(self.mMainPassCB), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), self.mDepthStencilBuffer.data_ptr(),
                              _ptr(src), _ptr(out), W, H, int(row0), int(H - row0 if rows is None else rows), gbuffer_flags(g),
                              None if params is None else C.byref(params), _stream(self.ctx.device)))
        return out

    def apply_fog(self, src=None, out=None, row0=0, rows=None, params=None):
        """crychic_fog on the context's stream: rows [row0, row0 + rows) of `out` from `src`, both (H, W, 4) uint8 tensors (default:
        mBackBuffer, in place; `out` alone given: from mBackBuffer into it; `src` alone given: in place on it), with this frame's depth
        plane, pass constants and cascade maps; params: a FogParams, None = the defaults.  Writes no other byte of `out`.  Returns
        `out`."""
        src, out, H, W = self._pass_frames("apply_fog", None, src, out)
        maps = (C.c_void_p * 4)(*[self.mShadowMap.mShadowMap[i].data_ptr() for i in range(4)])
        check(lib.crychic_fog(self.ctx.handle, C.byref(self.mMainPassCB), self.mDepthStencilBuffer.data_ptr(), maps, self.mShadowMap.Width(),
                              _ptr(src), _ptr(out), W, H, int(row0), int(H - row0 if rows is None else rows),
                              None if params is None else C.byref(params), _stream(self.ctx.device)))
        return out

    def set_decals(self, decals, textures=()):
        """The decals of apply_decals (extension): a sequence of at most MAX_DECALS Decal structs (geometry.decal_from_box), uploaded
        here, and the textures their indices address: at most DECAL_MAX_TEXTURES entries, each a (tensor, width, height, mipLevels)
        tuple as geometry.decal_texture returns -- a flat uint8 RGBA8 chain, uploaded here if it is not on the device -- or a Texture
        whose pointer the caller keeps alive.  An empty sequence clears them."""
        decals = list(decals)
        if len(decals) > _lib.MAX_DECALS or len(textures) > _lib.DECAL_MAX_TEXTURES:
            raise CrychicError(-1, "set_decals takes at most %d decals and %d textures" % (_lib.MAX_DECALS, _lib.DECAL_MAX_TEXTURES))
        self._decalKeep, table = [], (_lib.Texture * max(len(textures), 1))()
        for k, t in enumerate(textures):
            if isinstance(t, _lib.Texture):
                table[k] = t
                continue
            chain, w, h, levels = t
            chain = torch.as_tensor(chain).contiguous().view(torch.uint8).to(self.ctx.device)
            self._decalKeep.append(chain)
            table[k] = _lib.Texture(chain.data_ptr(), int(w), int(h), int(levels))
        self._decalTextures, self._decalTextureCount = table, len(textures)
        self.mDecalCount = len(decals)
        self.mDecals = None
        if decals:
            host = (_lib.Decal * len(decals))(*decals)
            self.mDecals = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(self.ctx.device)

    def apply_decals(self, row0=0, rows=None):
        """crychic_apply_decals on the context's stream: the decals of set_decals blended into rows [row0, row0 + rows) of
        mDeferred.mGBuffer, in the planes' formats, with this frame's depth plane and pass constants.  Explicit only: Draw() runs no
        producer passes here, so it cannot know whether the planes are fresh, and a second application stacks on the first."""
        n = self.mDecalCount
        g = self.mDeferred.mGBuffer
        H, W = self.mClientHeight, self.mClientWidth
        check(lib.crychic_apply_decals(self.ctx.handle, C.byref(self.mMainPassCB), self.mDepthStencilBuffer.data_ptr(), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                                       gbuffer_flags(g), self.mDecals.data_ptr() if n else None, n, self._decalTextures if n else None,
                                       self._decalTextureCount if n else 0, W, H, int(row0), int(H - row0 if rows is None else rows),
                                       _stream(self.ctx.device)))

    def antialias(self, src=None, out=None, row0=0, rows=None, params=None):
        """crychic_antialias on the context's stream: rows [row0, row0 + rows) of `out` (default: mBackBufferAA, allocated on first
        use) from `src` (default: mBackBuffer), both (H, W, 4) uint8 tensors; params: an AAParams, None = the defaults.  The pass reads
        rows [row0 - 16, row0 + rows + 16) of `src` and writes no other byte of `out`.  Returns `out`."""
        src, out, H, W = self._pass_frames("antialias", "mBackBufferAA", src, out, any_shape=True)
        check(lib.crychic_antialias(self.ctx.handle, _ptr(src), _ptr(out), W, H, int(row0), int(H - row0 if rows is None else rows),
                                    None if params is None else C.byref(params), _stream(self.ctx.device)))
        return out

    def set_cube_map(self, cube, dim=None, levels=1, gloss=False, ambient_sh=False, env_brdf=False, parallax=False):
        """The sky cube map: a 6 x dim x dim x 4 uint8 tensor (level 0 alone), or -- with `levels` > 1 -- the flat mip chain
        geometry.cube_mip_chain / load_dds_cube_mips produce (the reference binds the whole chain, CRYCHIC.cpp:1148-1151): the
        reflection and sky lookups are then trilinear (CRYCHIC_LIGHT_CUBE_LEVELS).  gloss (needs levels > 1): the chain is one
        prefilter_cube_map made, and the reflection lookup takes its level from the pixel's roughness (CRYCHIC_LIGHT_CUBE_GLOSS).
        ambient_sh (no chain, or a chain with gloss): the tensor holds geometry.cube_chain_sh_bytes(dim, levels) bytes, the cube map
        and behind it the environment tail project_irradiance filled; the ambient colour is then the SH9 irradiance along the
        pixel's normal instead of AmbientLight (CRYCHIC_LIGHT_AMBIENT_SH).  env_brdf (needs gloss): the tensor holds
        geometry.cube_chain_env_bytes(dim, levels) bytes, the chain, the environment tail and behind it the table build_env_brdf
        made; the reflection is then weighed by the split sum's second factor instead of shininess and the mirror direction's
        Fresnel term (CRYCHIC_LIGHT_ENV_BRDF).  parallax (needs gloss): the tensor holds at least
        geometry.cube_chain_sh_bytes(dim, levels) bytes and set_probe_volume (or capture_environment(probe_box=...)) wrote the probe
        volume into its environment tail; the reflection lookup is then box-projected through it (CRYCHIC_LIGHT_CUBE_PARALLAX)."""
        if gloss and int(levels) < 2:
            raise CrychicError(-1, "set_cube_map: gloss needs a chain (levels > 1)")
        from .geometry import cube_chain_env_bytes, cube_chain_sh_bytes

        def holds(option, nbytes, what):
            need = nbytes(int(dim) if dim is not None else int(cube.shape[1]), levels)
            if cube.numel() * cube.element_size() < need:
                raise CrychicError(-1, "set_cube_map: %s needs a tensor of %d bytes (%s)" % (option, need, what))
        if parallax:
            if not gloss:
                raise CrychicError(-1, "set_cube_map: parallax needs a prefiltered chain (levels > 1 and gloss=True)")
            holds("parallax", cube_chain_sh_bytes, "the chain and its environment tail")
        if env_brdf:
            if not gloss:
                raise CrychicError(-1, "set_cube_map: env_brdf needs a prefiltered chain (levels > 1 and gloss=True)")
            holds("env_brdf", cube_chain_env_bytes, "the chain, its environment tail and the table")
        if ambient_sh:
            if int(levels) > 1 and not gloss:
                raise CrychicError(-4, "set_cube_map: ambient_sh with a derivative-LOD chain is not supported (no chain, or gloss=True)")
            holds("ambient_sh", cube_chain_sh_bytes, "the cube map and its environment tail")
        self.mCubeMapGloss = bool(gloss)
        self.mCubeMapAmbientSH = bool(ambient_sh)
        self.mCubeMapEnvBrdf = bool(env_brdf)
        self.mCubeMapParallax = bool(parallax)
        self.mCubeMap = cube
        self.mCubeMapLevels = int(levels)
        self.mCubeMapSize = int(dim) if dim is not None else None
        self._desc = None

    def generate_cube_mips(self, chain, dim, levels=None):
        """Extension: builds levels 1 .. levels - 1 of the cube map chain in the uint8 tensor `chain` from its level 0, on the device and
        in place (crychic_generate_cube_mips; geometry.cube_mip_chain's bytes).  levels None = down to 1 x 1.  Returns `chain`."""
        from .geometry import cube_full_levels
        levels = cube_full_levels(dim) if levels is None else int(levels)
        check(lib.crychic_generate_cube_mips(self.ctx.handle, _ptr(chain), int(dim), levels, _stream(self.ctx.device)))
        return chain

    def prefilter_cube_map(self, chain, dim, levels, out=None):
        """Extension: the chain `chain` (a uint8 tensor: a box chain of generate_cube_mips or of a DDS file) prefiltered by roughness
        (crychic_prefilter_cube_chain; include/crychic_hip.h "prefiltered chain"): level 0 copied, level k convolved with the GGX
        lobe of roughness k / (levels - 1).  out: a uint8 tensor of at least geometry.cube_chain_bytes(dim, levels) bytes that does
        not overlap `chain` (default: a new one).  Returns `out`."""
        from .geometry import cube_chain_bytes
        nbytes = cube_chain_bytes(dim, levels)
        if out is None:
            out = torch.empty((nbytes,), device=self.ctx.device, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < nbytes or out.device != chain.device:
            raise CrychicError(-1, "prefilter_cube_map: out must be a contiguous uint8 device tensor of at least %d bytes" % nbytes)
        _check_chain("prefilter_cube_map", chain, nbytes)
        check(lib.crychic_prefilter_cube_chain(self.ctx.handle, _ptr(chain), _ptr(out), int(dim), int(levels), _stream(self.ctx.device)))
        return out

    def project_irradiance(self, chain, dim, levels, level=0):
        """Extension: projects level `level` of the cube map chain `chain` (a uint8 tensor of at least
        geometry.cube_chain_sh_bytes(dim, levels) bytes) onto the nine SH9 irradiance coefficients, into the chain's own environment
        tail at geometry.cube_sh_offset(dim, levels) (crychic_project_cube_sh; include/crychic_hip.h "SH9 irradiance").  Returns
        `chain`; set_cube_map(chain, dim, levels, ambient_sh=True) binds it."""
        from .geometry import cube_chain_bytes, cube_chain_sh_bytes, cube_sh_offset
        dim, levels, level = int(dim), int(levels), int(level)
        _check_chain("project_irradiance", chain, cube_chain_sh_bytes(dim, levels))
        if not 0 <= level < max(levels, 1):
            raise CrychicError(-1, "project_irradiance: level %d outside 0 .. %d" % (level, max(levels, 1) - 1))
        base = chain.data_ptr()
        check(lib.crychic_project_cube_sh(self.ctx.handle, C.c_void_p(base + (cube_chain_bytes(dim, level) if level else 0)),
                                          max(dim >> level, 1), C.c_void_p(base + cube_sh_offset(dim, levels)), _stream(self.ctx.device)))
        return chain

    def build_env_brdf(self, chain, dim, levels):
        """Extension: builds the 32 x 32 environment BRDF table of the split-sum specular term into the chain's own tensor (a uint8
        tensor of at least geometry.cube_chain_env_bytes(dim, levels) bytes), at geometry.cube_env_brdf_offset(dim, levels)
        (crychic_build_env_brdf; include/crychic_hip.h "environment BRDF table").  The table depends on nothing but its definition.
        Returns `chain`; set_cube_map(chain, dim, levels, gloss=True, env_brdf=True) binds it."""
        from .geometry import cube_chain_env_bytes, cube_env_brdf_offset
        dim, levels = int(dim), int(levels)
        _check_chain("build_env_brdf", chain, cube_chain_env_bytes(dim, levels))
        check(lib.crychic_build_env_brdf(self.ctx.handle, C.c_void_p(chain.data_ptr() + cube_env_brdf_offset(dim, levels)),
                                         _stream(self.ctx.device)))
        return chain

    def set_probe_volume(self, chain, dim, levels, pos, box_min, box_max):
        """Extension: writes the probe volume of the box-projected reflection lookup -- the capture position `pos` and the proxy box
        [box_min, box_max], three floats each, box_min < pos < box_max -- into the environment tail of `chain` (a uint8 tensor of at
        least geometry.cube_chain_sh_bytes(dim, levels) bytes), at geometry.cube_probe_offset(dim, levels)
        (crychic_set_cube_probe_volume; include/crychic_hip.h "probe volume").  Returns `chain`;
        set_cube_map(chain, dim, levels, gloss=True, parallax=True) binds it."""
        from .geometry import cube_chain_sh_bytes, cube_sh_offset
        dim, levels = int(dim), int(levels)
        _check_chain("set_probe_volume", chain, cube_chain_sh_bytes(dim, levels))
        v = [(C.c_float * 3)(*[float(x) for x in a]) for a in (pos, box_min, box_max)]
        check(lib.crychic_set_cube_probe_volume(self.ctx.handle, C.c_void_p(chain.data_ptr() + cube_sh_offset(dim, levels)), v[0], v[1], v[2],
                                                _stream(self.ctx.device)))
        return chain

    def capture_environment(self, pos, geometry, shadow_geometry=None, dim=256, levels=None, z_near=0.5, z_far=None, shadow_dim=1024,
                            out=None, prefilter=False, irradiance=False, env_brdf=False, probe_box=None):
        """Extension: renders the scene into a cube map at `pos` and builds its mip chain on the device (include/crychic_hip.h
        "environment capture").  Face f of level 0 is the frame Draw produces at dim x dim for face camera f
        (crychic_cube_capture_cameras) with CRYCHIC_LIGHT_SKY, written in place: `geometry` (a SceneGeometry) fills the normal map,
        depth and G-buffer, `shadow_geometry` (default: `geometry`) the four cascades fitted to that camera, in a shadow map of
        `shadow_dim` with pcfSearchRadius = crychic_pcf_search_radius(shadow_dim, self.pcfLiteral).  geometry None: no producer draws,
        the planes are cleared and every face is sky.  Lights[], AmbientLight, TotalTime, blurCount, numDirLights, the Q-fix flags,
        the point and spot lights with their shadow maps and ShadowTransforms[4..11], the SSAO offset vectors and the plane formats
        are this object's; the cube map it has bound is the source (with its chain), so a capture never reflects itself and two
        captures in a row give one bounce.  levels None = the full chain; z_far None = 100 (the reference's lens, CRYCHIC.cpp:114).
        out: a uint8 tensor of at least geometry.cube_chain_bytes(dim, levels) bytes that must not overlap the bound cube map
        (default: a new one).  The probe renderer is kept (release_capture_probes frees it), so a re-capture with `out` allocates nothing.  Returns (chain, dim, levels);
        binding it is the caller's set_cube_map(chain, dim, levels) -- with gloss=True for a prefiltered one.  prefilter: the chain returned is the captured box chain
        prefiltered by roughness (prefilter_cube_map); the box chain lives in a scratch tensor kept with the probes.  irradiance: the
        tensor returned has geometry.cube_chain_sh_bytes(dim, levels) bytes (so must `out`), and level 0 of the captured box chain is
        projected into its environment tail (project_irradiance) -- bind it with ambient_sh=True.  env_brdf (needs prefilter=True and
        more than one level): the tensor returned has geometry.cube_chain_env_bytes(dim, levels) bytes (so must `out`) and the
        environment BRDF table is built behind its environment tail (build_env_brdf) -- bind it with gloss=True, env_brdf=True.
        probe_box = (box_min, box_max) (needs prefilter=True and more than one level): the tensor returned has at least
        geometry.cube_chain_sh_bytes(dim, levels) bytes (so must `out`) and the probe volume -- this capture's `pos` and the box -- is
        written into the environment tail of the chain returned, the prefiltered one (set_probe_volume) -- bind it with gloss=True,
        parallax=True."""
        import numpy as np
        from .geometry import (cube_capture_cameras, cube_chain_bytes, cube_chain_env_bytes, cube_chain_sh_bytes, cube_env_brdf_offset,
                               cube_full_levels, cube_sh_offset)
        if env_brdf and not prefilter:
            raise CrychicError(-1, "capture_environment: env_brdf needs prefilter=True (the table weighs a prefiltered chain)")
        if probe_box is not None and not prefilter:
            raise CrychicError(-1, "capture_environment: probe_box needs prefilter=True (the box-projected lookup reads a prefiltered chain)")
        dim, shadow_dim = int(dim), int(shadow_dim)
        if not 0 < dim <= 8192:
            raise CrychicError(-1, "capture_environment: dim %d (a cube map the lighting pass binds has 2 .. 8192-texel faces)" % dim)
        full = cube_full_levels(dim)
        levels = full if levels is None else int(levels)
        if not 1 <= levels <= full:
            raise CrychicError(-1, "capture_environment: levels %d (1 .. %d for %d-texel faces)" % (levels, full, dim))
        if env_brdf and levels < 2:
            raise CrychicError(-1, "capture_environment: env_brdf needs a chain (levels > 1)")
        if probe_box is not None and levels < 2:
            raise CrychicError(-1, "capture_environment: probe_box needs a chain (levels > 1)")
        src = self.mCubeMap
        probe = self._probes.get((dim, shadow_dim))
        if probe is None:       # a dim x dim frame: an odd dim is refused as every frame size is (Ssao.OnResize)
            probe = self._probes[(dim, shadow_dim)] = Crychic(self.ctx, dim, dim, self.mSsao.mRandomVectorMap, src, shadow_dim=shadow_dim,
                                                              gbuffer_formats=self.mDeferred.mFormats)
        chain_bytes = cube_chain_bytes(dim, levels)
        nbytes = cube_chain_env_bytes(dim, levels) if env_brdf else cube_chain_sh_bytes(dim, levels) if irradiance or probe_box is not None else chain_bytes
        if out is None:
            out = torch.empty((nbytes,), device=self.ctx.device, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < nbytes or out.device != self.mBackBuffer.device:
            raise CrychicError(-1, "capture_environment: out must be a contiguous uint8 device tensor of at least %d bytes" % nbytes)
        if out.data_ptr() < src.data_ptr() + src.numel() * src.element_size() and src.data_ptr() < out.data_ptr() + nbytes:
            raise CrychicError(-1, "capture_environment: the destination aliases the bound cube map (a capture never reflects itself)")
        final = out
        if prefilter:           # the faces and their box chain go to the scratch chain, the prefiltered chain to `out`
            out = self._probe_chains.get((dim, levels))
            if out is None:
                out = self._probe_chains[(dim, levels)] = torch.empty((chain_bytes,), device=self.ctx.device, dtype=torch.uint8)
        if probe.mDeferred.mFormats != self.mDeferred.mFormats:
            probe.set_gbuffer_formats(self.mDeferred.mFormats)
        # the local lights' shadow maps are the main frame's: render them now if Draw has not yet
        if self._spotShadow is not None and self._spotShadow[3] is not None:
            self.DrawSpotShadowMaps()
        if self._pointShadow is not None and self._pointShadow[2] is not None:
            self.DrawPointShadowMaps()
        probe.mSsao.mRandomVectorMap = self.mSsao.mRandomVectorMap
        probe.mCubeMap, probe.mCubeMapLevels, probe.mCubeMapSize = src, self.mCubeMapLevels, self.mCubeMapSize
        probe.mCubeMapGloss = self.mCubeMapGloss        # a capture of a glossy scene is glossy
        probe.mCubeMapAmbientSH = self.mCubeMapAmbientSH  # ... and one lit by its environment is lit by it
        probe.mCubeMapEnvBrdf = self.mCubeMapEnvBrdf      # ... with the reflection weight the owner uses
        probe.mCubeMapParallax = self.mCubeMapParallax    # ... and the bound map's probe volume: it is stated in world space
        probe.blurCount, probe.numDirLights, probe.flags = self.blurCount, self.numDirLights, int(self.flags) | _lib.LIGHT_SKY
        probe.pcfSearchRadius = lib.crychic_pcf_search_radius(shadow_dim, int(self.pcfLiteral))
        probe.mPointLights, probe.mSpotLights = self.mPointLights, self.mSpotLights
        probe._spotShadow = None if self._spotShadow is None else self._spotShadow[:3] + (None,)
        probe._pointShadow = None if self._pointShadow is None else self._pointShadow[:2] + (None,)
        if geometry is None:
            probe.mDepthStencilBuffer.fill_(0xFFFFFF)
            probe.mSsao.mNormalMap.zero_()
            probe.mSsao.mNormalMap[..., 2] = 1.0
            for g in probe.mDeferred.mGBuffer:
                g.zero_()
            probe.mShadowMap.mShadowMap.fill_(0xFFFFFF)
        main = self.mMainPassCB
        cams = cube_capture_cameras(pos, z_near, 100.0 if z_far is None else z_far)
        light_dir = (C.c_float * 3)(*main.Lights[0].Direction)
        dirs = np.array([list(main.Lights[i].Direction) for i in range(3)], np.float32)
        lv, lp, st = (np.zeros((4, 4, 4), np.float32) for _ in range(3))
        for f in range(6):
            cam = cams[f]
            check(lib.crychic_update_cascade_shadow_transform(C.byref(cam), light_dir, shadow_dim, lv.ctypes.data, lp.ctypes.data, st.ctypes.data))
            pcb, scb = PassConstants(), SsaoConstants()
            check(lib.crychic_update_main_pass_cb(C.byref(cam), dim, dim, st.ctypes.data, dirs.ctypes.data, C.byref(pcb)))
            for i in range(_lib.MAX_LIGHTS):
                pcb.Lights[i] = main.Lights[i]
            pcb.AmbientLight[:] = main.AmbientLight[:]
            pcb.TotalTime, pcb.DeltaTime = main.TotalTime, main.DeltaTime
            for k in range(4, 12):
                pcb.ShadowTransforms[k][:] = main.ShadowTransforms[k][:]
            check(lib.crychic_update_ssao_cb(C.byref(cam), dim, dim, C.cast(self.mSsaoCB.OffsetVectors, C.c_void_p), C.byref(scb)))
            if geometry is not None:
                cbs = []
                for k in range(4):
                    vp = np.zeros((4, 4), np.float32)       # lightView * lightProj, summed term after term (UpdateShadowPassCB)
                    for q in range(4):
                        vp = vp + lv[k][:, q:q + 1] * lp[k][q:q + 1, :]
                    cb = PassConstants()
                    cb.ViewProj[:] = list(vp.T.reshape(-1))
                    cbs.append(cb)
                (shadow_geometry or geometry).DrawSceneToShadowMaps(cbs, [probe.mShadowMap.Resource(k) for k in range(4)])
                geometry.DrawNormalsDepthAndGBuffer(pcb, probe.mSsao.mNormalMap, probe.mDeferred.mGBuffer, probe.mDepthStencilBuffer)
            probe.mMainPassCB, probe.mSsaoCB = pcb, scb
            probe.mBackBuffer = out[f * dim * dim * 4:(f + 1) * dim * dim * 4].view(dim, dim, 4)
            probe.Draw()
        self.generate_cube_mips(out, dim, levels)
        if irradiance:          # the box chain's level 0 (the prefiltered chain's level 0 is its copy) into the tail of the chain returned
            check(lib.crychic_project_cube_sh(self.ctx.handle, _ptr(out), dim, C.c_void_p(final.data_ptr() + cube_sh_offset(dim, levels)),
                                              _stream(self.ctx.device)))
        if env_brdf:
            check(lib.crychic_build_env_brdf(self.ctx.handle, C.c_void_p(final.data_ptr() + cube_env_brdf_offset(dim, levels)),
                                             _stream(self.ctx.device)))
        if prefilter:
            out = self.prefilter_cube_map(out, dim, levels, out=final)
        if probe_box is not None:       # into the chain that is bound later: the prefiltered one
            self.set_probe_volume(final, dim, levels, pos, probe_box[0], probe_box[1])
        return out, dim, levels

    def render_sky(self, params=None, dim=256, levels=None, prefilter=False, irradiance=False, env_brdf=False, out=None):
        """Extension: renders the procedural sky -- a single-scattering atmosphere lit by the sun of `params` (a SkyParams; None = the
        defaults) -- into level 0 of a cube map (crychic_render_sky; include/crychic_hip.h "procedural sky") and builds what
        capture_environment builds behind a capture, in its order: the mip chain, then with irradiance the SH9 projection of level 0
        into the environment tail, with env_brdf (needs prefilter=True and more than one level) the environment BRDF table, with
        prefilter the chain prefiltered by roughness (the box chain lives in a scratch tensor kept with the capture probes).  levels
        None = the full chain.  out: a uint8 tensor of at least the bytes the options need (geometry.cube_chain_bytes,
        cube_chain_sh_bytes or cube_chain_env_bytes) that must not overlap the bound cube map (default: a new one).  Returns
        (chain, dim, levels); binding it is the caller's set_cube_map(chain, dim, levels, ...), as after a capture."""
        return self._render_sky(params, dim, levels, prefilter, irradiance, env_brdf, out, False)

    def _render_sky(self, params, dim, levels, prefilter, irradiance, env_brdf, out, own):
        """render_sky; own: `out` is followSun's own chain, which may be the bound one (the sky reads no cube map)."""
        from .geometry import cube_chain_bytes, cube_chain_env_bytes, cube_chain_sh_bytes, cube_env_brdf_offset, cube_full_levels, cube_sh_offset
        if env_brdf and not prefilter:
            raise CrychicError(-1, "render_sky: env_brdf needs prefilter=True (the table weighs a prefiltered chain)")
        dim = int(dim)
        if not 2 <= dim <= 8192:
            raise CrychicError(-1, "render_sky: dim %d (a sky cube map has 2 .. 8192-texel faces)" % dim)
        full = cube_full_levels(dim)
        levels = full if levels is None else int(levels)
        if not 1 <= levels <= full:
            raise CrychicError(-1, "render_sky: levels %d (1 .. %d for %d-texel faces)" % (levels, full, dim))
        if env_brdf and levels < 2:
            raise CrychicError(-1, "render_sky: env_brdf needs a chain (levels > 1)")
        chain_bytes = cube_chain_bytes(dim, levels)
        nbytes = cube_chain_env_bytes(dim, levels) if env_brdf else cube_chain_sh_bytes(dim, levels) if irradiance else chain_bytes
        if out is None:
            out = torch.empty((nbytes,), device=self.ctx.device, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < nbytes or out.device != self.mBackBuffer.device:
            raise CrychicError(-1, "render_sky: out must be a contiguous uint8 device tensor of at least %d bytes" % nbytes)
        src = self.mCubeMap
        if not own and out.data_ptr() < src.data_ptr() + src.numel() * src.element_size() and src.data_ptr() < out.data_ptr() + nbytes:
            raise CrychicError(-1, "render_sky: the destination aliases the bound cube map")
        final = out
        if prefilter:           # the faces and their box chain go to the scratch chain, the prefiltered chain to `out`
            out = self._probe_chains.get((dim, levels))
            if out is None:
                out = self._probe_chains[(dim, levels)] = torch.empty((chain_bytes,), device=self.ctx.device, dtype=torch.uint8)
        check(lib.crychic_render_sky(self.ctx.handle, _ptr(out), dim, 0, 6, None if params is None else C.byref(params), _stream(self.ctx.device)))
        self.skyRenders += 1
        if levels > 1:
            self.generate_cube_mips(out, dim, levels)
        if irradiance:
            check(lib.crychic_project_cube_sh(self.ctx.handle, _ptr(out), dim, C.c_void_p(final.data_ptr() + cube_sh_offset(dim, levels)),
                                              _stream(self.ctx.device)))
        if env_brdf:
            check(lib.crychic_build_env_brdf(self.ctx.handle, C.c_void_p(final.data_ptr() + cube_env_brdf_offset(dim, levels)),
                                             _stream(self.ctx.device)))
        if prefilter:
            out = self.prefilter_cube_map(out, dim, levels, out=final)
        return out, dim, levels

    @staticmethod
    def sky_sun_colour(params=None):
        """Extension: the colour of the sun's light under the sky of `params` (crychic_sky_sun_colour): three floats, the sun's
        intensity through the atmosphere along its own ray, zeros when the planet hides it -- what Lights[0].Strength should be so
        that the light reddens as the sky does.  Host code; needs no device."""
        rgb = (C.c_float * 3)()
        check(lib.crychic_sky_sun_colour(None if params is None else C.byref(params), rgb))
        return tuple(rgb)

    def _follow_sun(self):
        """Draw() with followSun set: the sun of the sky is where Lights[0] shines from.  If that direction or the parameters are not
        those of the sky last rendered, or another cube map was bound since, the sky is rendered anew -- with the mips, the prefilter,
        the SH projection and the table that the flags of the last set_cube_map need -- into a chain of this object's own, which is
        then bound with those flags."""
        p = SkyParams.from_buffer_copy(self._followSun) if isinstance(self._followSun, SkyParams) else SkyParams.default()
        d = self.mMainPassCB.Lights[0].Direction
        p.sunDir[:] = [-d[0], -d[1], -d[2]]
        if self.mCubeMapParallax:
            raise CrychicError(-1, "followSun: a sky has no probe volume (set_cube_map(parallax=True) is bound)")
        dim, levels = int(self.mCubeMapSize or self.mCubeMap.shape[1]), int(self.mCubeMapLevels)
        flags = (self.mCubeMapGloss, self.mCubeMapAmbientSH, self.mCubeMapEnvBrdf)
        key = (bytes(p), dim, levels, flags)
        if key == self._skyKey and self._skyChain is not None and self.mCubeMap.data_ptr() == self._skyChain.data_ptr():
            return
        from .geometry import cube_chain_env_bytes
        nbytes = cube_chain_env_bytes(dim, levels)      # room for the tail and the table, whatever the flags
        if self._skyChain is None or self._skyChain.numel() != nbytes:
            self._skyChain = torch.empty((nbytes,), device=self.ctx.device, dtype=torch.uint8)
        self._render_sky(p, dim, levels, flags[0], flags[1], flags[2], self._skyChain, True)
        self.set_cube_map(self._skyChain, dim, levels, gloss=flags[0], ambient_sh=flags[1], env_brdf=flags[2])
        self._skyKey = key

    @property
    def followSun(self):
        """Extension: None | True | SkyParams.  When set, Draw() takes the sky's sunDir from -mMainPassCB.Lights[0].Direction in front
        of the lighting frame and re-renders the procedural sky (render_sky) whenever the direction or the parameters changed, into a
        chain of its own, bound with the flags the previous set_cube_map asked for.  Independent of the passes behind the lighting
        pass and of strips: every rank renders the same deterministic cube.  Unset, Draw issues exactly the calls it issues without it."""
        return self._followSun

    @followSun.setter
    def followSun(self, value):
        if not (value is None or value is True or value is False or isinstance(value, SkyParams)):
            raise CrychicError(-1, "followSun: None, True or a SkyParams")
        self._followSun = value or None
        self._skyKey = None

    def release_capture_probes(self):
        """Frees the probe renderers capture_environment keeps (one per (dim, shadow_dim) it was called with)."""
        self._probes.clear()
        self._probe_chains.clear()

    def set_point_lights(self, lights):
        """Extension: `lights` is a ctypes array of Light (or None); copied to the device.  Shadows set with set_point_shadows are
        dropped (their transforms belong to the previous lights)."""
        if lights is None or len(lights) == 0:
            self.mPointLights = None
            self._pointHost = None
        else:
            import numpy as np
            host = np.frombuffer(bytes(lights), dtype=np.uint8).copy()
            self.mPointLights = torch.from_numpy(host).to(self.ctx.device)
            self._pointHost = (Light * len(lights)).from_buffer_copy(bytes(lights))
        self.mPointShadowMaps = None
        self._pointShadow = None
        self._desc = None

    def set_spot_lights(self, lights):
        """Extension: `lights` is a ctypes array of Light (or None); copied to the device.  Spot lights are lit after the point
        lights (include/crychic_hip.h crychic_deferred_light_spots); None or an empty array = none.  Shadows set with
        set_spot_shadows are dropped (their transforms belong to the previous lights)."""
        if lights is None or len(lights) == 0:
            self.mSpotLights = None
            self._spotHost = None
        else:
            import numpy as np
            host = np.frombuffer(bytes(lights), dtype=np.uint8).copy()
            self.mSpotLights = torch.from_numpy(host).to(self.ctx.device)
            self._spotHost = (Light * len(lights)).from_buffer_copy(bytes(lights))
        self.mSpotShadowMaps = None
        self._spotShadow = None
        self._desc = None

    def set_spot_shadows(self, count, dim=1024, fov_y=math.pi / 2, z_near=0.5, geometry=None):
        """Extension: the first `count` (<= 8) spot lights cast shadows (include/crychic_hip.h crychic_deferred_light_spots_shadowed).
        Allocates `count` dim x dim D24 maps, builds each light's transform (crychic_update_spot_shadow_transform: perspective, fov_y,
        z_near .. FalloffEnd) and from then on every Draw writes it into ShadowTransforms[4 + k] and passes the
        maps' descriptor (mMainPassCB itself is not modified).  geometry (a SceneGeometry of the shadow casters): Draw renders the maps first,
        in one DrawSceneToShadowMaps call, after whatever the caller drew for the cascades; without it the caller fills mSpotShadowMaps
        (DrawSpotShadowMaps renders them on demand).  count 0 removes the shadows."""
        if count == 0:
            self.mSpotShadowMaps, self._spotShadow = None, None
            return
        n = 0 if self._spotHost is None else len(self._spotHost)
        if not 0 < count <= 8 or count > n:
            raise CrychicError(-1, "set_spot_shadows: count %d (1 .. 8, at most the %d spot lights)" % (count, n))
        if not 2 <= dim <= 16384:
            raise CrychicError(-1, "set_spot_shadows: dim %d (2 .. 16384)" % dim)
        import numpy as np
        T, cbs = [], []
        for k in range(count):
            lv, lp, st = ((C.c_float * 16)() for _ in range(3))
            check(lib.crychic_update_spot_shadow_transform(C.byref(self._spotHost[k]), float(fov_y), float(z_near), lv, lp, st))
            T.append(list(np.asarray(st[:], np.float32).reshape(4, 4).T.reshape(-1)))
            cb = PassConstants()
            vp = np.asarray(lv[:], np.float32).reshape(4, 4) @ np.asarray(lp[:], np.float32).reshape(4, 4)
            cb.ViewProj[:] = list(vp.astype(np.float32).T.reshape(-1))
            cbs.append(cb)
        self.mSpotShadowMaps = torch.full((count, dim, dim), 0xFFFFFF, dtype=torch.int32, device=self.ctx.device)
        desc = SpotShadows()
        desc.count, desc.dim = count, dim
        for k in range(count):
            desc.maps[k] = self.mSpotShadowMaps[k].data_ptr()
        self._spotShadow = (desc, T, cbs, geometry)

    def spot_shadow_pass_constants(self):
        """The shadow pass constants (ViewProj = lightView * lightProj) of the shadowed spot lights, in map order."""
        return [] if self._spotShadow is None else list(self._spotShadow[2])

    def DrawSpotShadowMaps(self, geometry=None):
        """Renders every spot shadow map in one crychic_draw_scene_to_shadow_maps pass (the cascades' rasteriser and bias)."""
        desc, T, cbs, geo = self._spotShadow
        geo = geometry if geometry is not None else geo
        geo.DrawSceneToShadowMaps(cbs, [self.mSpotShadowMaps[k] for k in range(len(cbs))])

    def set_point_shadows(self, count, dim=512, z_near=0.5, geometry=None):
        """Extension: the first `count` (<= 4) point lights cast cube shadows (include/crychic_hip.h crychic_deferred_light_point_shadows).
        Allocates mPointShadowMaps, (count, 6, dim, dim) D24 faces cleared to 1.0, builds each light's face views and shadow projection
        (crychic_update_point_shadow_transforms: widened 90-degree faces, z_near .. FalloffEnd) and from then on every Draw
        passes their descriptor.  geometry (a SceneGeometry of the shadow casters): Draw renders the faces first
        (DrawPointShadowMaps); without it the caller fills mPointShadowMaps.  count 0 removes the shadows."""
        if count == 0:
            self.mPointShadowMaps, self._pointShadow = None, None
            return
        n = 0 if self._pointHost is None else len(self._pointHost)
        if not 0 < count <= 4 or count > n:
            raise CrychicError(-1, "set_point_shadows: count %d (1 .. 4, at most the %d point lights)" % (count, n))
        if not 16 <= dim <= 16384:
            raise CrychicError(-1, "set_point_shadows: dim %d (16 .. 16384)" % dim)
        import numpy as np
        desc = PointShadows()
        desc.count, desc.dim = count, dim
        cbs = []
        for k in range(count):
            lv, lp, sp = ((C.c_float * 16) * 6)(), (C.c_float * 16)(), (C.c_float * 16)()
            check(lib.crychic_update_point_shadow_transforms(C.byref(self._pointHost[k]), int(dim), float(z_near), lv, lp, sp))
            desc.shadowProj[k][:] = sp[:]
            for f in range(6):
                cb = PassConstants()
                vp = np.asarray(lv[f][:], np.float32).reshape(4, 4) @ np.asarray(lp[:], np.float32).reshape(4, 4)
                cb.ViewProj[:] = list(vp.astype(np.float32).T.reshape(-1))
                cbs.append(cb)
        self.mPointShadowMaps = torch.full((count, 6, dim, dim), 0xFFFFFF, dtype=torch.int32, device=self.ctx.device)
        for k in range(count):
            desc.maps[k] = self.mPointShadowMaps[k].data_ptr()
        self._pointShadow = (desc, cbs, geometry)

    def point_shadow_pass_constants(self):
        """The shadow pass constants (ViewProj = lightView[f] * lightProj) of the shadowed point lights' faces: light-major, faces
        +X, -X, +Y, -Y, +Z, -Z."""
        return [] if self._pointShadow is None else list(self._pointShadow[1])

    def DrawPointShadowMaps(self, geometry=None):
        """Renders every point shadow face with crychic_draw_scene_to_shadow_maps (the cascades' rasteriser and bias), at most 12
        faces (two lights) per call."""
        desc, cbs, geo = self._pointShadow
        geo = geometry if geometry is not None else geo
        faces = [self.mPointShadowMaps[k, f] for k in range(len(cbs) // 6) for f in range(6)]
        for i in range(0, len(cbs), 12):
            geo.DrawSceneToShadowMaps(cbs[i:i + 12], faces[i:i + 12])

    def set_profiling(self, enabled):
        check(lib.crychic_ctx_set_profiling(self.ctx.handle, 1 if enabled else 0))

    def blur_chain_timed_out(self):
        """crychic_blur_chain_status: True if a workgroup of the most recent single-launch blur chain gave up waiting for a neighbour
        (synchronises the stream; the frame's ambient map would be wrong)."""
        flag = C.c_uint32(0)
        check(lib.crychic_blur_chain_status(self.ctx.handle, _stream(self.ctx.device), C.byref(flag)))
        return bool(flag.value)

    def last_pass_times(self):
        t = PassTimes()
        check(lib.crychic_ctx_last_pass_times(self.ctx.handle, C.byref(t)))
        return {"ssao_ms": t.ssao_ms, "blur_ms": t.blur_ms, "light_ms": t.light_ms, "total_ms": t.total_ms}


class SceneGeometry:
    """Device-resident vertex / index / instance / material / texture buffers of a set of render items, i.e. what
    CRYCHIC::BuildShapeGeometry + BuildMaterials + the per-frame InstanceBuffers hold (CRYCHIC.cpp:1250-1445, 515-592)."""

    def __init__(self, ctx, items, materials=None, textures=None):
        import numpy as np
        dev = ctx.device
        self.ctx = ctx
        self._keep = []
        self.items = (DrawItem * len(items))()
        self.triangles = 0
        uploads = {}

        def upload(a, as_type):
            # None or an empty array: a null buffer.  An array object that several items pass (a shared vertex buffer) is uploaded
            # once: the key is the caller's own object, which `uploads` keeps alive, never a temporary copy.
            if a is None or len(a) == 0:
                return None
            if id(a) not in uploads:
                t = torch.from_numpy(np.ascontiguousarray(a).view(as_type).copy()).to(dev)
                uploads[id(a)] = (a, t)
                self._keep.append(t)
            return uploads[id(a)][1]

        for k, item in enumerate(items):
            # (vertices, indices, instances) or (vertices, indices, instances, startIndexLocation, baseVertexLocation): with the two
            # locations the item draws the indices from startIndexLocation to the end of the array it is given
            v, idx, inst = item[:3]
            start, base = (int(item[3]), int(item[4])) if len(item) == 5 else (0, 0)
            count = (len(idx) if idx is not None else 0) - start
            tv, ti, tn = upload(v, np.uint8), upload(idx, np.int32), upload(inst, np.uint8)
            self.items[k] = DrawItem(tv.data_ptr() if tv is not None else None, len(v) if v is not None else 0,
                                     ti.data_ptr() if ti is not None else None, count, start, base,
                                     tn.data_ptr() if tn is not None else None, len(inst) if inst is not None else 0)
            self.triangles += (count // 3) * (len(inst) if inst is not None else 0)
        self.materials = None
        self.n_materials = 0
        if materials is not None:
            self.materials = torch.from_numpy(np.ascontiguousarray(materials).view(np.uint8).copy()).to(dev)
            self.n_materials = len(materials)
        self.textures = None
        self.n_textures = 0
        if textures:
            self.textures = (Texture * len(textures))()
            for k, t in enumerate(textures):
                if t is None:
                    continue
                from .geometry import texture_levels
                flat, tw, th, levels = texture_levels(t)          # one array = level 0 only; a list = a mip chain
                tt = torch.from_numpy(flat.copy()).to(dev)
                self._keep.append(tt)
                self.textures[k] = Texture(tt.data_ptr(), tw, th, levels)
            self.n_textures = len(textures)
        self._ws = {}

    def workspace(self, W, H, targets=1):
        key = (W, H, targets)
        if key not in self._ws:
            n = int(lib.crychic_raster_workspace_bytes(self.triangles * targets, W, H))
            self._ws[key] = torch.zeros((n,), dtype=torch.uint8, device=self.ctx.device)
        return self._ws[key]

    def DrawSceneToShadowMap(self, pass_cb, shadow_plane, depth_bias=10000, slope_bias=2.0):  # CRYCHIC.cpp:2477-2510, 1601-1603
        dim = int(shadow_plane.shape[0])
        ws = self.workspace(dim, dim)
        check(lib.crychic_draw_scene_to_shadow_map(self.ctx.handle, C.byref(pass_cb), self.items, len(self.items), _ptr(shadow_plane), dim,
                                                   int(depth_bias), float(slope_bias), _ptr(ws), ws.numel(), _stream(self.ctx.device)))

    def DrawSceneToShadowMaps(self, pass_cbs, shadow_planes, depth_bias=10000, slope_bias=2.0):
        """All cascades in one rasteriser pass (crychic_draw_scene_to_shadow_maps); bit-identical to one call per cascade."""
        n = len(pass_cbs)
        dim = int(shadow_planes[0].shape[0])
        ws = self.workspace(dim, dim, n)
        cbs = (type(pass_cbs[0]) * n)(*pass_cbs)
        ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in shadow_planes])
        check(lib.crychic_draw_scene_to_shadow_maps(self.ctx.handle, C.cast(cbs, C.c_void_p), n, self.items, len(self.items), C.cast(ptrs, C.c_void_p), dim,
                                                    int(depth_bias), float(slope_bias), _ptr(ws), ws.numel(), _stream(self.ctx.device)))

    def DrawNormalsAndDepth(self, pass_cb, normal_map, depth):  # CRYCHIC.cpp:2512-2543
        H, W = int(depth.shape[0]), int(depth.shape[1])
        ws = self.workspace(W, H)
        check(lib.crychic_draw_normals_and_depth(self.ctx.handle, C.byref(pass_cb), self.items, len(self.items), _ptr(normal_map), _ptr(depth),
                                                 W, H, _ptr(ws), ws.numel(), _stream(self.ctx.device)))

    def DrawNormalsDepthAndGBuffer(self, pass_cb, normal, gbuffer, depth, g_rows=None):
        """DrawNormalsAndDepth + DrawGBuffer on one rasterisation (same items, same ViewProj => same visibility); every plane is
        bit-identical to the two separate passes.  g_rows = (row0, rows): a rank's strip -- depth and normals for the whole
        frame, G0..G2 for those rows only."""
        if normal is None:      # the library would take it for the G-buffer pass alone
            raise CrychicError(-1, "null normal / G-buffer target")
        self._draw_camera_pass(pass_cb, normal, gbuffer, depth, g_rows)

    def DrawGBuffer(self, pass_cb, gbuffer, depth, g_rows=None):  # CRYCHIC.cpp:2545-2571; g_rows = (row0, rows): scissored to a strip
        self._draw_camera_pass(pass_cb, None, gbuffer, depth, g_rows)

    def _draw_camera_pass(self, pass_cb, normal, gbuffer, depth, g_rows):
        """crychic_draw_gbuffer_formats, the G-buffer producers in one: normal None = the G-buffer pass alone, otherwise the fused
        pass; each plane's format is its tensor's dtype.  The entry reads 0 rows as the whole target, so an explicit g_rows with 0
        rows is refused here, as the _rows entries refuse it."""
        H, W = int(depth.shape[0]), int(depth.shape[1])
        r0, rn = (0, 0) if g_rows is None else (int(g_rows[0]), int(g_rows[1]))
        if g_rows is not None and rn == 0:
            raise CrychicError(-1, "G-buffer rows [%u,+%u) outside the %u-row target" % (r0, rn, H))
        ws = self.workspace(W, H)
        check(lib.crychic_draw_gbuffer_formats(self.ctx.handle, C.byref(pass_cb), self.items, len(self.items), _ptr(self.materials),
                                               self.n_materials, self.textures, self.n_textures, _ptr(normal), _ptr(gbuffer[0]), _ptr(gbuffer[1]),
                                               _ptr(gbuffer[2]), gbuffer_flags(gbuffer), _ptr(depth), W, H, r0, rn, _ptr(ws), ws.numel(),
                                               _stream(self.ctx.device)))
