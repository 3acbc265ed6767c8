"""ctypes binding of libcrychic_hip.so (include/crychic_hip.h).

The library is the product: if it has not been built (python -m crychic_renderer_amd.build, or
__graft_entry__.build()) importing this module raises -- there is no Python or CPU fallback.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# CRYCHIC_LIB: a probe build of the same library (tools/probes/variants.sh builds them with extra -D flags); never set in tests or bench runs
LIB_PATH = os.environ.get("CRYCHIC_LIB") or os.path.join(HERE, "libcrychic_hip.so")

MAX_LIGHTS = 16
LIGHT_SKY = 1
LIGHT_CUBE_GLOSS = 0x800      # CRYCHIC_LIGHT_CUBE_GLOSS: the bound chain is prefiltered by roughness
LIGHT_AMBIENT_SH = 0x8000     # CRYCHIC_LIGHT_AMBIENT_SH: the ambient colour from the SH9 coefficients behind the cube map
LIGHT_ENV_BRDF = 0x100000     # CRYCHIC_LIGHT_ENV_BRDF: the reflection weighed by the environment BRDF table behind the environment tail
LIGHT_CUBE_PARALLAX = 0x200000    # CRYCHIC_LIGHT_CUBE_PARALLAX: the reflection lookup box-projected through the probe volume in the environment tail
CUBE_PROBE_OFFSET, CUBE_PROBE_BYTES = 368, 48     # CRYCHIC_CUBE_PROBE_OFFSET / _BYTES: the probe volume inside the environment tail
ENV_BRDF_BYTES = 4096         # CRYCHIC_ENV_BRDF_BYTES: 32 x 32 dwords A | B << 16
CUBE_SH_BYTES = 512           # CRYCHIC_CUBE_SH_BYTES: the environment tail (144 bytes of coefficients, then the projection's scratch)
# CRYCHIC_GBUFFER_G*_F16: that G-buffer plane holds half4 texels (the flags word of the lighting entries, FrameDesc.flags, and
# crychic_draw_gbuffer_formats' gbufferFlags)
GBUFFER_G0_F16, GBUFFER_G1_F16, GBUFFER_G2_F16 = 0x1000, 0x2000, 0x4000
GBUFFER_F16_MASK = 0x7000
COMM_ID_BYTES = 128
AA_MAX_SEARCH = 16            # CRYCHIC_AA_MAX_SEARCH: the longest end search of crychic_antialias, in pixels
FOG_MAX_STEPS = 64            # CRYCHIC_FOG_MAX_STEPS: the most samples crychic_fog takes along a view ray
SKY_MAX_VIEW_STEPS, SKY_MAX_SUN_STEPS = 64, 32      # CRYCHIC_SKY_MAX_VIEW_STEPS, CRYCHIC_SKY_MAX_SUN_STEPS: the marches of crychic_render_sky
SSR_MAX_STEPS = 64            # CRYCHIC_SSR_MAX_STEPS: the most samples crychic_ssr takes along a reflected ray
DOF_MAX_RADIUS = 8            # CRYCHIC_DOF_MAX_RADIUS: the largest gather radius of crychic_dof, in pixels
BLOOM_MAX_LEVELS = 8          # CRYCHIC_BLOOM_MAX_LEVELS: the most levels of crychic_bloom's pyramid
SHARPEN_MAX_STRENGTH, SHARPEN_MAX_LIMIT = 256, 3584      # CRYCHIC_SHARPEN_MAX_STRENGTH, CRYCHIC_SHARPEN_MAX_LIMIT (Q12) of crychic_sharpen
GRADE_MAX_N = 33              # CRYCHIC_GRADE_MAX_N: the largest table of crychic_grade (33 x 33 x 33 entries: 143 748 bytes of LDS)


class Light(C.Structure):
    _fields_ = [("Strength", C.c_float * 3), ("FalloffStart", C.c_float), ("Direction", C.c_float * 3),
                ("FalloffEnd", C.c_float), ("Position", C.c_float * 3), ("SpotPower", C.c_float)]


class PassConstants(C.Structure):
    _fields_ = [("View", C.c_float * 16), ("InvView", C.c_float * 16), ("Proj", C.c_float * 16),
                ("InvProj", C.c_float * 16), ("ViewProj", C.c_float * 16), ("InvViewProj", C.c_float * 16),
                ("ViewProjTex", C.c_float * 16), ("ShadowTransforms", (C.c_float * 16) * 12),
                ("EyePosW", C.c_float * 3), ("cbPerObjectPad1", C.c_float), ("RenderTargetSize", C.c_float * 2),
                ("InvRenderTargetSize", C.c_float * 2), ("NearZ", C.c_float), ("FarZ", C.c_float),
                ("TotalTime", C.c_float), ("DeltaTime", C.c_float), ("AmbientLight", C.c_float * 4),
                ("Lights", Light * MAX_LIGHTS)]


class SsaoConstants(C.Structure):
    _fields_ = [("Proj", C.c_float * 16), ("InvProj", C.c_float * 16), ("ProjTex", C.c_float * 16),
                ("OffsetVectors", (C.c_float * 4) * 14), ("BlurWeights", (C.c_float * 4) * 3),
                ("RenderTargetSize", C.c_float * 2), ("InvRenderTargetSize", C.c_float * 2),
                ("OcclusionRadius", C.c_float), ("OcclusionFadeStart", C.c_float), ("OcclusionFadeEnd", C.c_float),
                ("SurfaceEpsilon", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("look", C.c_float * 3), ("up", C.c_float * 3), ("fovY", C.c_float),
                ("aspect", C.c_float), ("nearZ", C.c_float), ("farZ", C.c_float)]


class FrameDesc(C.Structure):
    _fields_ = [("W", C.c_uint32), ("H", C.c_uint32), ("blurCount", C.c_int), ("numDirLights", C.c_int),
                ("pcfSearchRadius", C.c_float), ("flags", C.c_uint32), ("row0", C.c_uint32), ("rows", C.c_uint32),
                ("normal_dev", C.c_void_p), ("depth_dev", C.c_void_p), ("randvec_dev", C.c_void_p),
                ("g0_dev", C.c_void_p), ("g1_dev", C.c_void_p), ("g2_dev", C.c_void_p),
                ("shadow_dev", C.c_void_p * 4), ("shadowDim", C.c_uint32), ("cube_dev", C.c_void_p),
                ("cubeDim", C.c_uint32), ("ambient0_dev", C.c_void_p), ("ambient1_dev", C.c_void_p),
                ("edge_dev", C.c_void_p), ("out_rgba8_dev", C.c_void_p),
                ("point_lights_dev", C.c_void_p), ("numPointLights", C.c_uint32)]


class DrawItem(C.Structure):
    _fields_ = [("vertices_dev", C.c_void_p), ("vertexCount", C.c_uint32), ("indices_dev", C.c_void_p), ("indexCount", C.c_uint32),
                ("startIndexLocation", C.c_uint32), ("baseVertexLocation", C.c_int32), ("instances_dev", C.c_void_p),
                ("instanceCount", C.c_uint32)]


class Texture(C.Structure):
    _fields_ = [("rgba8_dev", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("mipLevels", C.c_uint32)]


class SpotShadows(C.Structure):
    """crychic_spot_shadows: the first `count` spot lights read maps[k] through ShadowTransforms[4 + k] (extension)."""
    _fields_ = [("count", C.c_uint32), ("dim", C.c_uint32), ("maps", C.c_void_p * 8)]


class PointShadows(C.Structure):
    """crychic_point_shadows: the first `count` point lights read the six faces at maps[k] through shadowProj[k] (extension)."""
    _fields_ = [("count", C.c_uint32), ("dim", C.c_uint32), ("maps", C.c_void_p * 4), ("shadowProj", (C.c_float * 16) * 4)]


class AAParams(C.Structure):
    """crychic_aa_params: the knobs of crychic_antialias (extension); AAParams.default() = crychic_aa_default_params."""
    _fields_ = [("absMin", C.c_uint32), ("relShift", C.c_uint32), ("searchSteps", C.c_uint32), ("subpix", C.c_uint32)]

    @classmethod
    def default(cls, **fields):
        p = cls()
        check(lib.crychic_aa_default_params(C.byref(p)))
        for k, v in fields.items():
            setattr(p, k, int(v))
        return p


class FogParams(C.Structure):
    """crychic_fog_params: the knobs of crychic_fog (extension); FogParams.default() = crychic_fog_default_params.  ambient and sun
    take an (R, G, B) sequence."""
    _fields_ = [("density", C.c_float), ("maxDistance", C.c_float), ("steps", C.c_uint32), ("ambient", C.c_uint8 * 4), ("sun", C.c_uint8 * 4),
                ("reserved", C.c_uint32 * 3)]

    @classmethod
    def default(cls, **fields):
        p = cls()
        check(lib.crychic_fog_default_params(C.byref(p)))
        for k, v in fields.items():
            if k in ("ambient", "sun"):
                setattr(p, k, (C.c_uint8 * 4)(*[int(c) for c in tuple(v)[:3]]))
            elif k == "steps":
                p.steps = int(v)
            else:
                setattr(p, k, float(v))
        return p


class SkyParams(C.Structure):
    """crychic_sky_params: the knobs of crychic_render_sky (extension); SkyParams.default() = crychic_sky_default_params.  sunDir
    takes an (x, y, z) sequence, towards the sun; the definition normalises it."""
    _fields_ = [("sunDir", C.c_float * 3), ("altitude", C.c_float), ("sunIntensity", C.c_float), ("exposure", C.c_float),
                ("sunAngularRadius", C.c_float), ("groundAlbedo", C.c_float), ("viewSteps", C.c_uint32), ("sunSteps", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]

    @classmethod
    def default(cls, **fields):
        p = cls()
        check(lib.crychic_sky_default_params(C.byref(p)))
        for k, v in fields.items():
            if k == "sunDir":
                p.sunDir = (C.c_float * 3)(*[float(c) for c in v])
            elif k == "reserved":
                p.reserved = (C.c_uint32 * 2)(*[int(c) for c in v])
            else:
                setattr(p, k, int(v) if k in ("viewSteps", "sunSteps") else float(v))
        return p


class SsrParams(C.Structure):
    """crychic_ssr_params: the knobs of crychic_ssr (extension); SsrParams.default() = crychic_ssr_default_params."""
    _fields_ = [("maxDistance", C.c_float), ("thickness", C.c_float), ("bias", C.c_float), ("maxRoughness", C.c_float), ("steps", C.c_uint32),
                ("edgeFade", C.c_uint32), ("intensity", C.c_uint32), ("reserved", C.c_uint32)]

    @classmethod
    def default(cls, **fields):
        p = cls()
        check(lib.crychic_ssr_default_params(C.byref(p)))
        for k, v in fields.items():
            setattr(p, k, int(v) if k in ("steps", "edgeFade", "intensity", "reserved") else float(v))
        return p


SSR_GLOSS_MAX_LEVELS = 8       # CRYCHIC_SSR_GLOSS_MAX_LEVELS: the most levels, the frame included, of crychic_ssr_pyramid


class SsrGlossParams(C.Structure):
    """crychic_ssr_gloss_params: the cone of crychic_ssr_glossy (extension); SsrGlossParams.default() = crychic_ssr_gloss_default_params."""
    _fields_ = [("coneScale", C.c_float), ("levels", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    @classmethod
    def default(cls, **fields):
        p = cls()
        check(lib.crychic_ssr_gloss_default_params(C.byref(p)))
        for k, v in fields.items():
            if k == "reserved":
                p.reserved = (C.c_uint32 * 2)(*[int(c) for c in v])
            else:
                setattr(p, k, int(v) if k == "levels" else float(v))
        return p


assert C.sizeof(SsrGlossParams) == 16


class DofParams(C.Structure):
    """crychic_dof_params: the knobs of crychic_dof (extension); DofParams.default() = crychic_dof_default_params, with focus, aperture
    and radius as short names of focusDistance, aperture and maxRadius."""
    _fields_ = [("focusDistance", C.c_float), ("aperture", C.c_float), ("maxRadius", C.c_uint32), ("reserved", C.c_uint32 * 5)]

    @classmethod
    def default(cls, focus=None, aperture=None, radius=None):
        p = cls()
        check(lib.crychic_dof_default_params(C.byref(p)))
        if focus is not None:
            p.focusDistance = float(focus)
        if aperture is not None:
            p.aperture = float(aperture)
        if radius is not None:
            p.maxRadius = int(radius)
        return p


MAX_DECALS, DECAL_MAX_TEXTURES = 64, 16       # CRYCHIC_MAX_DECALS, CRYCHIC_DECAL_MAX_TEXTURES
DECAL_ALBEDO, DECAL_ROUGHNESS, DECAL_METALNESS, DECAL_NORMAL = 1, 2, 4, 8
DECAL_NO_TEXTURE = 0xFFFFFFFF


class Decal(C.Structure):
    """crychic_decal (160 bytes): an oriented box that blends a texture into the G-buffer planes (extension; crychic_apply_decals).
    geometry.decal_from_box fills one from a matrix."""
    _fields_ = [("invWorld", C.c_float * 12), ("boundsMin", C.c_float * 3), ("boundsMax", C.c_float * 3), ("tangentW", C.c_float * 3),
                ("bitangentW", C.c_float * 3), ("normalW", C.c_float * 3), ("tint", C.c_float * 3), ("opacity", C.c_float),
                ("roughness", C.c_float), ("metalness", C.c_float), ("fadeScale", C.c_float), ("fadeBias", C.c_float),
                ("texelsPerUnit", C.c_float), ("texture", C.c_uint32), ("normalTexture", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(Decal) == 160


class BloomParams(C.Structure):
    """crychic_bloom_params: the knobs of crychic_bloom (extension); BloomParams.default() = crychic_bloom_default_params, any field
    replaced by its keyword."""
    _fields_ = [("threshold", C.c_uint32), ("knee", C.c_uint32), ("scatter", C.c_uint32), ("intensity", C.c_uint32), ("levels", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]

    @classmethod
    def default(cls, threshold=None, knee=None, scatter=None, intensity=None, levels=None):
        p = cls()
        check(lib.crychic_bloom_default_params(C.byref(p)))
        for name, v in (("threshold", threshold), ("knee", knee), ("scatter", scatter), ("intensity", intensity), ("levels", levels)):
            if v is not None:
                setattr(p, name, int(v))
        return p


class GradeParams(C.Structure):
    """crychic_grade_params: an ASC CDL (slope, offset, power per channel) and a saturation, what crychic_grade_build_lut makes a
    table of (extension); GradeParams.default() = crychic_grade_default_params -- the identity --, any field replaced by its keyword
    (slope, offset and power: one number for all three channels, or three)."""
    _fields_ = [("slope", C.c_float * 3), ("offset", C.c_float * 3), ("power", C.c_float * 3), ("saturation", C.c_float)]

    @classmethod
    def default(cls, slope=None, offset=None, power=None, saturation=None):
        p = cls()
        check(lib.crychic_grade_default_params(C.byref(p)))
        for name, v in (("slope", slope), ("offset", offset), ("power", power)):
            if v is not None:
                getattr(p, name)[:] = [float(v)] * 3 if isinstance(v, (int, float)) else [float(c) for c in v]
        if saturation is not None:
            p.saturation = float(saturation)
        return p


assert C.sizeof(GradeParams) == 40


class SharpenParams(C.Structure):
    """crychic_sharpen_params: the knobs of crychic_sharpen (extension); SharpenParams.default() = crychic_sharpen_default_params, any
    field replaced by its keyword."""
    _fields_ = [("strength", C.c_uint32), ("limit", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    @classmethod
    def default(cls, strength=None, limit=None):
        p = cls()
        check(lib.crychic_sharpen_default_params(C.byref(p)))
        for name, v in (("strength", strength), ("limit", limit)):
            if v is not None:
                setattr(p, name, int(v))
        return p


assert C.sizeof(SharpenParams) == 16


TAA_RESET, TAA_NO_CLAMP = 1, 2               # CRYCHIC_TAA_RESET, CRYCHIC_TAA_NO_CLAMP


class TaaParams(C.Structure):
    """crychic_taa_params: the knobs of crychic_taa (extension); TaaParams.default() = crychic_taa_default_params, any field replaced by
    its keyword."""
    _fields_ = [("blend", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 6)]

    @classmethod
    def default(cls, blend=None, flags=None):
        p = cls()
        check(lib.crychic_taa_default_params(C.byref(p)))
        if blend is not None:
            p.blend = int(blend)
        if flags is not None:
            p.flags = int(flags)
        return p


class TaaUpscaleParams(C.Structure):
    """crychic_taa_upscale_params: the knobs of crychic_taa_upscale (extension; the flags are TAA_RESET and TAA_NO_CLAMP);
    TaaUpscaleParams.default() = crychic_taa_upscale_default_params, any field replaced by its keyword."""
    _fields_ = [("blend", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 6)]

    @classmethod
    def default(cls, blend=None, flags=None):
        p = cls()
        check(lib.crychic_taa_upscale_default_params(C.byref(p)))
        if blend is not None:
            p.blend = int(blend)
        if flags is not None:
            p.flags = int(flags)
        return p


class MotionBlurParams(C.Structure):
    """crychic_motion_blur_params: the knobs of crychic_motion_blur (extension); MotionBlurParams.default() =
    crychic_motion_blur_default_params, any field replaced by its keyword."""
    _fields_ = [("shutter", C.c_uint32), ("samples", C.c_uint32), ("maxRadius", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]

    @classmethod
    def default(cls, shutter=None, samples=None, maxRadius=None, flags=None):
        p = cls()
        check(lib.crychic_motion_blur_default_params(C.byref(p)))
        for name, v in (("shutter", shutter), ("samples", samples), ("maxRadius", maxRadius), ("flags", flags)):
            if v is not None:
                setattr(p, name, int(v))
        return p


class PassTimes(C.Structure):
    _fields_ = [("ssao_ms", C.c_float), ("blur_ms", C.c_float), ("light_ms", C.c_float), ("total_ms", C.c_float)]


assert C.sizeof(Light) == 48 and C.sizeof(PassConstants) == 2048 and C.sizeof(SsaoConstants) == 496

_u32, _i, _f, _vp, _sz = C.c_uint32, C.c_int, C.c_float, C.c_void_p, C.c_size_t
_P = C.POINTER

# name -> (restype, argtypes); every symbol include/crychic_hip.h declares
PROTOTYPES = {
    "crychic_ctx_create": (_i, [_i, _P(_vp)]),
    "crychic_ctx_destroy": (None, [_vp]),
    "crychic_last_error": (C.c_char_p, []),
    "crychic_version": (C.c_char_p, []),
    "crychic_ctx_device_name": (C.c_char_p, [_vp]),
    "crychic_calc_gauss_weights": (_i, [_f, _P(_f), _i]),
    "crychic_msvc_rand": (_i, [_P(_u32)]),
    "crychic_build_offset_vectors": (None, [_P(_u32), _P(C.c_float * 4)]),
    "crychic_build_random_vector_texture": (None, [_P(_u32), _i, _vp]),
    "crychic_update_cascade_shadow_transform": (_i, [_P(Camera), _P(_f), _u32, _vp, _vp, _vp]),
    "crychic_update_spot_shadow_transform": (_i, [_P(Light), _f, _f, _vp, _vp, _vp]),
    "crychic_update_point_shadow_transforms": (_i, [_P(Light), _u32, _f, _vp, _vp, _vp]),
    "crychic_update_main_pass_cb": (_i, [_P(Camera), _u32, _u32, _vp, _vp, _P(PassConstants)]),
    "crychic_update_ssao_cb": (_i, [_P(Camera), _u32, _u32, _vp, _P(SsaoConstants)]),
    "crychic_pcf_search_radius": (_f, [_u32, _i]),
    "crychic_edge_plane_bytes": (_sz, [_u32, _u32]),
    "crychic_ssao": (_i, [_vp, _P(SsaoConstants), _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp]),
    "crychic_ssao_edges": (_i, [_vp, _P(SsaoConstants), _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp]),
    "crychic_ssao_blur": (_i, [_vp, _P(SsaoConstants), _vp, _vp, _vp, _u32, _u32, _i, _u32, _u32, _vp]),
    "crychic_ssao_compute": (_i, [_vp, _P(SsaoConstants), _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _i, _u32, _u32,
                                  _vp]),
    "crychic_deferred_light": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _P(_vp), _u32, _vp, _u32, _vp,
                                    _vp, _u32, _u32, _u32, _u32, _i, _f, _u32, _vp]),
    "crychic_deferred_light_points": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _P(_vp), _u32, _vp, _u32, _vp,
                                           _vp, _u32, _u32, _u32, _u32, _i, _f, _u32, _vp, _u32, _vp]),
    "crychic_draw_hot_path": (_i, [_vp, _P(SsaoConstants), _P(PassConstants), _P(FrameDesc), _vp]),
    "crychic_deferred_light_spots": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _P(_vp), _u32, _vp, _u32, _vp,
                                          _vp, _u32, _u32, _u32, _u32, _i, _f, _u32, _vp, _u32, _vp, _u32, _vp]),
    "crychic_draw_hot_path_spots": (_i, [_vp, _P(SsaoConstants), _P(PassConstants), _P(FrameDesc), _vp, _u32, _vp]),
    "crychic_deferred_light_spots_shadowed": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _P(_vp), _u32, _vp, _u32, _vp,
                                                   _vp, _u32, _u32, _u32, _u32, _i, _f, _u32, _vp, _u32, _vp, _u32, _P(SpotShadows),
                                                   _vp]),
    "crychic_draw_hot_path_spots_shadowed": (_i, [_vp, _P(SsaoConstants), _P(PassConstants), _P(FrameDesc), _vp, _u32,
                                                  _P(SpotShadows), _vp]),
    "crychic_deferred_light_point_shadows": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _P(_vp), _u32, _vp, _u32, _vp,
                                                  _vp, _u32, _u32, _u32, _u32, _i, _f, _u32, _vp, _u32, _vp, _u32, _P(SpotShadows),
                                                  _P(PointShadows), _vp]),
    "crychic_draw_hot_path_point_shadows": (_i, [_vp, _P(SsaoConstants), _P(PassConstants), _P(FrameDesc), _vp, _u32,
                                                 _P(SpotShadows), _P(PointShadows), _vp]),
    "crychic_frustum_cull": (_i, [_P(Camera), _P(_f), _P(_f), _vp, _u32, _vp]),
    "crychic_ctx_set_profiling": (_i, [_vp, _i]),
    "crychic_ctx_last_pass_times": (_i, [_vp, _P(PassTimes)]),
    "crychic_strip_rows": (_i, [_u32, _i, _i, _P(_u32), _P(_u32)]),
    "crychic_comm_unique_id": (_i, [_vp]),
    "crychic_comm_create": (_i, [_vp, _i, _i, _vp, _P(_vp)]),
    "crychic_comm_create_all": (_i, [_P(_vp), _i, _P(_vp)]),
    "crychic_comm_destroy": (None, [_vp]),
    "crychic_comm_abort": (_i, [_vp]),
    "crychic_comm_rank": (_i, [_vp]),
    "crychic_comm_size": (_i, [_vp]),
    "crychic_comm_async_error": (_i, [_vp]),
    "crychic_allgather_frame": (_i, [_vp, _vp, _u32, _u32, _P(_u32), _vp]),
    "crychic_allgather_frame_all": (_i, [_P(_vp), _i, _P(_vp), _u32, _u32, _P(_u32), _P(_vp)]),
    "crychic_comm_barrier": (_i, [_vp, _vp]),
    "crychic_draw_hot_path_shared": (_i, [_vp, _P(SsaoConstants), _P(PassConstants), _P(FrameDesc), _P(_u32), _u32, _vp]),
    "crychic_draw_hot_path_shared_spots": (_i, [_vp, _P(SsaoConstants), _P(PassConstants), _P(FrameDesc), _P(_u32), _u32, _vp, _u32,
                                                _vp]),
    "crychic_draw_hot_path_shared_spots_shadowed": (_i, [_vp, _P(SsaoConstants), _P(PassConstants), _P(FrameDesc), _P(_u32), _u32,
                                                         _vp, _u32, _P(SpotShadows), _vp]),
    "crychic_draw_hot_path_shared_point_shadows": (_i, [_vp, _P(SsaoConstants), _P(PassConstants), _P(FrameDesc), _P(_u32), _u32,
                                                        _vp, _u32, _P(SpotShadows), _P(PointShadows), _vp]),
    "crychic_create_box": (_i, [_f, _f, _f, _u32, _vp, _u32, _vp, _u32, _P(_u32)]),
    "crychic_create_grid": (_i, [_f, _f, _u32, _u32, _vp, _u32, _vp, _u32, _P(_u32)]),
    "crychic_load_mesh_text": (_i, [C.c_char_p, _vp, _u32, _vp, _u32, _P(_u32), _P(_u32)]),
    "crychic_load_dds_rgba8": (_i, [C.c_char_p, _vp, _sz, _P(_u32), _P(_u32)]),
    "crychic_load_dds_rgba8_mips": (_i, [C.c_char_p, _vp, _sz, _P(_u32), _P(_u32), _P(_u32)]),
    "crychic_load_dds_cube_rgba8": (_i, [C.c_char_p, _vp, _sz, _P(_u32)]),
    "crychic_load_dds_cube_rgba8_mips": (_i, [C.c_char_p, _vp, C.c_size_t, _P(_u32), _P(_u32)]),
    "crychic_cube_chain_bytes": (_sz, [_u32, _u32]),
    "crychic_generate_cube_mips": (_i, [_vp, _vp, _u32, _u32, _vp]),
    "crychic_cube_capture_cameras": (_i, [_P(_f), _f, _f, _P(Camera)]),
    "crychic_cube_prefilter_samples": (_i, [_u32, _u32, _u32, _vp, _P(_u32), _P(_f)]),
    "crychic_prefilter_cube_chain": (_i, [_vp, _vp, _vp, _u32, _u32, _vp]),
    "crychic_cube_sh_offset": (_sz, [_u32, _u32]),
    "crychic_cube_chain_sh_bytes": (_sz, [_u32, _u32]),
    "crychic_project_cube_sh": (_i, [_vp, _vp, _u32, _vp, _vp]),
    "crychic_cube_env_brdf_offset": (_sz, [_u32, _u32]),
    "crychic_cube_chain_env_bytes": (_sz, [_u32, _u32]),
    "crychic_build_env_brdf": (_i, [_vp, _vp, _vp]),
    "crychic_cube_probe_offset": (_sz, [_u32, _u32]),
    "crychic_set_cube_probe_volume": (_i, [_vp, _vp, _P(_f), _P(_f), _P(_f), _vp]),
    "crychic_sky_default_params": (_i, [_P(SkyParams)]),
    "crychic_render_sky": (_i, [_vp, _vp, _u32, _u32, _u32, _P(SkyParams), _vp]),
    "crychic_sky_sun_colour": (_i, [_P(SkyParams), _P(_f)]),
    "crychic_aa_default_params": (_i, [_P(AAParams)]),
    "crychic_antialias": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _P(AAParams), _vp]),
    "crychic_fog_default_params": (_i, [_P(FogParams)]),
    "crychic_fog": (_i, [_vp, _P(PassConstants), _vp, _P(_vp), _u32, _vp, _vp, _u32, _u32, _u32, _u32, _P(FogParams), _vp]),
    "crychic_ssr_default_params": (_i, [_P(SsrParams)]),
    "crychic_ssr": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _P(SsrParams), _vp]),
    "crychic_ssr_gloss_default_params": (_i, [_P(SsrGlossParams)]),
    "crychic_ssr_pyramid_bytes": (_sz, [_u32, _u32, _u32]),
    "crychic_ssr_pyramid_offset": (_sz, [_u32, _u32, _u32, _u32]),
    "crychic_ssr_pyramid": (_i, [_vp, _vp, _u32, _u32, _u32, _vp, _sz, _vp]),
    "crychic_ssr_glossy": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _u32, _u32, _u32, _u32, _u32, _P(SsrParams),
                                _P(SsrGlossParams), _vp]),
    "crychic_dof_default_params": (_i, [_P(DofParams)]),
    "crychic_dof": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _u32, _u32, _u32, _u32, _P(DofParams), _vp]),
    "crychic_decal_from_box": (_i, [_P(_f), _u32, _u32, _f, _f, _P(Decal)]),
    "crychic_apply_decals": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _u32, _vp, _u32, _P(Texture), _u32, _u32, _u32, _u32, _u32, _vp]),
    "crychic_bloom_default_params": (_i, [_P(BloomParams)]),
    "crychic_bloom_workspace_bytes": (_sz, [_u32, _u32, _u32]),
    "crychic_bloom_level_offset": (_sz, [_u32, _u32, _u32, _u32]),
    "crychic_bloom_pyramid": (_i, [_vp, _vp, _u32, _u32, _P(BloomParams), _vp, _sz, _vp]),
    "crychic_bloom_composite": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _P(BloomParams), _vp, _sz, _vp]),
    "crychic_bloom": (_i, [_vp, _vp, _vp, _u32, _u32, _P(BloomParams), _vp, _sz, _vp]),
    "crychic_grade_default_params": (_i, [_P(GradeParams)]),
    "crychic_grade_build_lut": (_i, [_P(GradeParams), _u32, _vp, _sz]),
    "crychic_load_cube_lut": (_i, [C.c_char_p, _vp, _sz, _P(C.c_uint32)]),
    "crychic_grade": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _u32, _vp]),
    "crychic_sharpen_default_params": (_i, [_P(SharpenParams)]),
    "crychic_sharpen": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _P(SharpenParams), _vp]),
    "crychic_taa_jitter": (_i, [_u32, _P(_f), _P(_f)]),
    "crychic_update_main_pass_cb_jittered": (_i, [_P(Camera), _u32, _u32, _vp, _vp, _f, _f, _P(PassConstants)]),
    "crychic_update_ssao_cb_jittered": (_i, [_P(Camera), _u32, _u32, _vp, _f, _f, _P(SsaoConstants)]),
    "crychic_taa_default_params": (_i, [_P(TaaParams)]),
    "crychic_taa_history_bytes": (_sz, [_u32, _u32]),
    "crychic_motion_blur_default_params": (_i, [_P(MotionBlurParams)]),
    "crychic_motion_blur_workspace_bytes": (_sz, [_u32, _u32]),
    "crychic_motion_blur_tile_offset": (_sz, [_u32, _u32]),
    "crychic_motion_blur_velocity": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _u32, _u32, _P(MotionBlurParams), _vp, _sz, _vp]),
    "crychic_motion_blur_gather": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _P(MotionBlurParams), _vp, _sz, _vp]),
    "crychic_motion_blur": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _u32, _u32, _P(MotionBlurParams), _vp, _sz, _vp]),
    "crychic_taa": (_i, [_vp, _P(PassConstants), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _P(TaaParams), _vp]),
    "crychic_taa_upscale_default_params": (_i, [_P(TaaUpscaleParams)]),
    "crychic_taa_upscale": (_i, [_vp, _P(PassConstants), _vp, _vp, _f, _f, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _u32, _u32, _u32,
                                 _P(TaaUpscaleParams), _vp]),
    "crychic_save_ppm":(_i, [C.c_char_p, _vp, _u32, _u32]),
    "crychic_raster_workspace_bytes": (_sz, [C.c_uint64, _u32, _u32]),
    "crychic_raster_status": (_i, [_vp, _vp, _P(_u32)]),
    "crychic_blur_chain_status": (_i, [_vp, _vp, _P(_u32)]),
    "crychic_draw_scene_to_shadow_map": (_i, [_vp, _P(PassConstants), _P(DrawItem), _u32, _vp, _u32, _i, _f, _vp, _sz, _vp]),
    "crychic_draw_scene_to_shadow_maps": (_i, [_vp, _vp, _u32, _P(DrawItem), _u32, _vp, _u32, _i, _f, _vp, _sz, _vp]),
    "crychic_draw_normals_and_depth": (_i, [_vp, _P(PassConstants), _P(DrawItem), _u32, _vp, _vp, _u32, _u32, _vp, _sz, _vp]),
    "crychic_draw_gbuffer": (_i, [_vp, _P(PassConstants), _P(DrawItem), _u32, _vp, _u32, _P(Texture), _u32, _vp, _vp, _vp, _vp,
                                  _u32, _u32, _vp, _sz, _vp]),
    "crychic_draw_normals_depth_and_gbuffer": (_i, [_vp, _P(PassConstants), _P(DrawItem), _u32, _vp, _u32, _P(Texture), _u32, _vp, _vp, _vp, _vp, _vp,
                                               _u32, _u32, _vp, _sz, _vp]),
    "crychic_draw_gbuffer_rows": (_i, [_vp, _P(PassConstants), _P(DrawItem), _u32, _vp, _u32, _P(Texture), _u32, _vp, _vp, _vp, _vp,
                                       _u32, _u32, _u32, _u32, _vp, _sz, _vp]),
    "crychic_draw_normals_depth_and_gbuffer_rows": (_i, [_vp, _P(PassConstants), _P(DrawItem), _u32, _vp, _u32, _P(Texture), _u32, _vp, _vp, _vp, _vp,
                                                        _vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp]),
    "crychic_gbuffer_plane_bytes": (_sz, [_u32, _u32, _u32, _i]),
    "crychic_draw_gbuffer_formats": (_i, [_vp, _P(PassConstants), _P(DrawItem), _u32, _vp, _u32, _P(Texture), _u32, _vp, _vp, _vp, _vp,
                                          _u32, _vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp]),
}


class CrychicError(RuntimeError):
    """Mirror of the reference's DxException (Common/d3dUtil.h:132-144) for a failed C-ABI call."""

    def __init__(self, status, what):
        super().__init__("crychic status %d: %s" % (status, what))
        self.status = status


def _preload_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so (same soname as /opt/rocm's).  Device pointers handed to the C
    ABI come from torch's allocator, so both must live in ONE HIP runtime: load torch's copy first, then the
    dynamic linker resolves libcrychic_hip.so's NEEDED libamdhip64.so.7 to it by soname.  Without torch (pure C++
    callers) the library simply binds to /opt/rocm's runtime."""
    try:
        import torch  # noqa: F401  (imports its bundled runtime)
    except ImportError:
        return
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load():
    _preload_hip_runtime()
    # Rebuild a missing / stale library when the toolchain is present (a checkout whose sources are newer than the .so);
    # this is a build step, not a fallback: without hipcc and without a library the import fails below.
    try:
        from . import build as _build
        if _build._stale() and os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            _build.build(verbose=False)
    except Exception as e:  # a failed rebuild must not be hidden behind an old binary
        if os.path.exists(LIB_PATH):
            raise ImportError("libcrychic_hip.so is stale and rebuilding it failed: %s" % e)
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libcrychic_hip.so is not built (%s). Run `python -m crychic_renderer_amd.build`; "
            "crychic_renderer_amd has no CPU/Python fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = load()


def check(status):
    if status < 0:
        raise CrychicError(status, lib.crychic_last_error().decode("utf-8", "replace"))
    return status
