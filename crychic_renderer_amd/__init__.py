"""crychic_renderer_amd -- MI355X (gfx950) backend for CRYCHIC's per-pixel hot path.

Package layout (only what the path needs):
  csrc/            hand-written HIP kernels, the extern "C" ABI (include/crychic_hip.h) and host constant builders
  _lib.py          ctypes binding of libcrychic_hip.so (raises if the library is not built: no fallback)
  renderer.py      Python mirror of the reference's pass objects (Ssao, DeferredShading, ShadowMap, CRYCHIC.Draw)
  scene.py         synthetic input planes
  geometry.py      meshes / instances / materials of the reference scene for the producer passes (row f1)
  sharding.py      multi-GPU row-strip plan + RCCL all-gather of the composed frame
"""
from ._lib import (AAParams, AA_MAX_SEARCH, FogParams, FOG_MAX_STEPS, SkyParams, SKY_MAX_VIEW_STEPS, SKY_MAX_SUN_STEPS, SsrParams, SSR_MAX_STEPS, SsrGlossParams, SSR_GLOSS_MAX_LEVELS, DofParams, DOF_MAX_RADIUS, BloomParams, BLOOM_MAX_LEVELS, GradeParams, GRADE_MAX_N, SharpenParams, SHARPEN_MAX_STRENGTH, SHARPEN_MAX_LIMIT, TaaParams, TaaUpscaleParams, MotionBlurParams, TAA_RESET, TAA_NO_CLAMP, Decal, MAX_DECALS, DECAL_MAX_TEXTURES, DECAL_ALBEDO, DECAL_ROUGHNESS, DECAL_METALNESS, DECAL_NORMAL, DECAL_NO_TEXTURE, CrychicError, Camera, FrameDesc, Light, PassConstants, PassTimes, SsaoConstants, LIGHT_SKY, LIGHT_CUBE_GLOSS, LIGHT_AMBIENT_SH, LIGHT_ENV_BRDF, LIGHT_CUBE_PARALLAX,
                   GBUFFER_G0_F16, GBUFFER_G1_F16, GBUFFER_G2_F16, GBUFFER_F16_MASK, check, lib)  # noqa: F401
from .renderer import Context, Ssao, DeferredShading, ShadowMap, Crychic, SceneGeometry, gbuffer_formats, gbuffer_flags  # noqa: F401
