"""python -m crychic_renderer_amd.demo [--size WxH] [--out frame.ppm] [--textures DIR] [--cube FILE.dds] [--gbuffer f32|mixed|f16]
                                   [--capture-env X,Y,Z [--capture-dim N]] [--gloss] [--env-ambient] [--env-specular]
                                   [--probe-box X0,Y0,Z0,X1,Y1,Z1] [--aa]
                                   [--ssr [--ssr-steps N] [--ssr-distance X] [--ssr-max-roughness X]
                                          [--ssr-gloss [--ssr-cone X] [--ssr-levels N]]]
                                   [--fog [--fog-density X] [--fog-steps N]]
                                   [--dof [--dof-focus X] [--dof-aperture X] [--dof-radius N]]
                                   [--bloom [--bloom-threshold N] [--bloom-intensity N] [--bloom-levels N]]
                                   [--taa [--taa-frames N]] [--taa-upscale WxH [--taa-frames N]]
                                   [--motion-blur [--motion-blur-shutter N] [--motion-blur-samples N] [--motion-blur-pan DX]]
                                   [--sharpen [--sharpen-strength N]]
                                   [--grade-cube FILE.cube | --grade-slope R,G,B --grade-offset R,G,B --grade-power R,G,B --grade-saturation X]

Renders one frame of the reference's live scene entirely on the GPU -- 4 shadow cascades, view normals + depth, G-buffer
(HIP rasteriser), SSAO + blur, deferred lighting + sky -- and writes it as PPM (the headless stand-in for Present).
--capture-env: before the frame, the scene is rendered into a cube map at X,Y,Z (Crychic.capture_environment: six faces of
--capture-dim texels and their mip chain, built on the device) and the frame is rendered with that chain bound, so the boxes and the
grid show up in the reflections.
--gloss (with --cube or --capture-env): the chain is prefiltered by roughness on the device (Crychic.prefilter_cube_map; a --cube file
without a chain gets its box chain first) and bound with glossy reflections, so a rough surface shows a blurred environment.
--env-ambient (with --cube or --capture-env): level 0 of the cube map is projected onto SH9 irradiance coefficients on the device
(Crychic.project_irradiance / capture_environment(irradiance=True)) and the ambient term takes its colour from them along the pixel's
normal instead of the constant AmbientLight: a floor is tinted by the sky above it and by the box beside it.  Without --gloss the cube
map is bound as level 0 alone (the derivative-LOD chain has no such kernels).
--env-specular (with --gloss): the environment BRDF table is built on the device behind the chain (Crychic.build_env_brdf /
capture_environment(env_brdf=True)) and the glossy reflection is weighed by the split sum's second factor instead of
(1 - roughness) times the mirror direction's Fresnel term: a rough metal keeps its brightness head-on, a rough dielectric its grazing
sheen.
--probe-box (with --capture-env and --gloss): the axis-aligned proxy box of the captured surroundings.  The capture writes its
position and the box into the chain's environment tail (capture_environment(probe_box=...)) and the reflection lookup is box-projected
through it (set_cube_map(parallax=True)): a box's reflection in the floor meets the box at its foot instead of sliding with the
camera.
--aa: the finished frame goes through the post-process anti-aliasing pass (Crychic.antiAliasing = True: crychic_antialias after the
lighting pass, the deferred path's stand-in for the framework's 4x MSAA switch) and the anti-aliased buffer is what is written.
--ssr: screen-space reflections of the lit frame (Crychic.ssr: crychic_ssr after the lighting pass, in front of --fog and every other
stage, into a buffer of its own on which the fog then works): a smooth surface shows what stands on it, blended over the cube-map
reflection; --ssr-steps (samples along each ray, default 32, at most 64), --ssr-distance (the ray's length in world units, default 20)
and --ssr-max-roughness (surfaces at or above it do not reflect, default 0.75) set its parameters.
--ssr-gloss (needs --ssr; experimental): the hit colour comes from a blurred pyramid of the lit frame, at the level whose texel is as
wide as the reflection cone at the hit (Crychic.ssrGloss: crychic_ssr_pyramid and crychic_ssr_glossy in place of crychic_ssr);
--ssr-cone (the cone's width per unit of roughness, 0 .. 16; the default 0 is the sharp pass, 0.7 a measured starting point) and
--ssr-levels (the pyramid's levels, the frame counted, 1 .. 8, default 6) set its parameters.
--fog: volumetric fog with sun shafts through the cascade maps (Crychic.fog: crychic_fog after the lighting pass, in place on the back
buffer, in front of --aa); --fog-density (default 0.02) and --fog-steps (default 16, at most 64) set its parameters.
--dof: depth of field from the depth plane (Crychic.depthOfField: crychic_dof after the lighting pass and the fog, in front of --aa);
--dof-focus (the distance in focus, default 15), --dof-aperture (the blur radius in pixels of a point at infinity, default 6, at most
64) and --dof-radius (the gather radius in pixels, default 8, at most 8) set its parameters.  The PPM is the last stage's output.
--bloom: what lies over a luma threshold is spread down and up a pyramid and added back (Crychic.bloom: crychic_bloom after the lighting
pass, the fog and --dof, in front of --aa); --bloom-threshold (8-bit luma, default 192), --bloom-intensity (256 = 1.0, default 128, at
most 1024) and --bloom-levels (default 6, at most 8) set its parameters.
--taa: temporal anti-aliasing (Crychic.temporalAA: crychic_taa after the lighting pass and the fog, in front of --dof, --bloom and
--aa): --taa-frames frames (default 16) of the still scene are rendered, each with the projection shifted by its sub-pixel jitter
(crychic_taa_jitter), and blended into the history; the resolved frame of the last one is what the later stages read.
--taa-upscale WxH: temporal upsampling (Crychic.temporalUpscale: crychic_taa_upscale at --taa's place, not together with --taa, --dof or
--motion-blur): --taa-frames jittered frames (default 16) of the still scene are rendered at --size and accumulated into a history of
W x H pixels, each side 1 to 4 times --size's; --bloom and --aa then run at W x H, and the PPM has that size.
--motion-blur: camera-motion blur (Crychic.motionBlur: crychic_motion_blur behind --dof, in front of --bloom and --aa): the frame is
drawn as if the camera had stood --motion-blur-pan world units (default 0.5) further along +x one frame earlier, and blurred along the
velocity that gives each pixel through its depth; --motion-blur-shutter (exposure in 1/256 of the frame interval, default 128, at
most 256) and --motion-blur-samples (2, 4, 8, 16 or 32, default 8) set its parameters.  With --taa the last frame is the one that moved.
--decals: deferred decals between the G-buffer pass and the lighting pass (Crychic.set_decals / apply_decals: crychic_apply_decals): a
glossy puddle with a dent normal map on the floor and a painted ring on the face of a box.
--grade-cube FILE.cube, or any of --grade-slope, --grade-offset, --grade-power (R,G,B or one number for all three) and
--grade-saturation: the colour grade (Crychic.colourGrade: crychic_grade behind --bloom, in front of --aa): the frame's look through a
3D table, loaded from an Adobe / Resolve .cube file or built from an ASC CDL with a saturation at 33 x 33 x 33 entries.
--grade-saturation 0 writes a grey frame.
--sharpen: contrast-adaptive sharpening (Crychic.sharpening: crychic_sharpen directly behind --taa or --taa-upscale, then at the display
size, and in front of --dof); --sharpen-strength (0 .. 256, default: the measured one of crychic_sharpen_default_params) sets how much
of the limited weight is used."""
import argparse
import ctypes as C
import math

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--out", default="frame.ppm")
    ap.add_argument("--shadow-dim", type=int, default=2048)
    ap.add_argument("--textures", default="", help="directory with the reference's DDS textures (else procedural stand-ins)")
    ap.add_argument("--cube", default="", help="a DDS cube map for the sky and the reflections, e.g. the reference's Textures/snowcube1024.dds "
                                               "(else a procedural one)")
    ap.add_argument("--gbuffer", default="f32", choices=["f32", "mixed", "f16"],
                    help="G-buffer plane formats: f32 = three float4 planes, mixed = G0 float4 with G1 and G2 half4, f16 = all three half4")
    ap.add_argument("--capture-env", default="", metavar="X,Y,Z", help="capture the environment at this position before the frame and render "
                                                                       "with the captured cube map bound")
    ap.add_argument("--capture-dim", type=int, default=256, help="face size of the captured cube map (even)")
    ap.add_argument("--gloss", action="store_true", help="prefilter the cube map chain by roughness and render glossy reflections "
                                                         "(needs --cube or --capture-env)")
    ap.add_argument("--env-ambient", action="store_true", help="ambient light from the cube map's SH9 irradiance instead of the constant "
                                                               "(needs --cube or --capture-env)")
    ap.add_argument("--env-specular", action="store_true", help="weigh the glossy reflection by the environment BRDF table (needs --gloss)")
    ap.add_argument("--probe-box", default="", metavar="X0,Y0,Z0,X1,Y1,Z1", help="box-project the captured reflections through this box around "
                                                                                 "the capture position (needs --capture-env and --gloss)")
    ap.add_argument("--aa", action="store_true", help="anti-alias the finished frame (post-process pass) and write the anti-aliased buffer")
    ap.add_argument("--ssr", action="store_true", help="screen-space reflections of the lit frame, after the lighting pass and in front of the fog")
    ap.add_argument("--ssr-steps", type=int, default=None, metavar="N", help="samples along each reflected ray, 1 .. 64 (default 32; needs --ssr)")
    ap.add_argument("--ssr-distance", type=float, default=None, metavar="X", help="length of a reflected ray in world units (default 20; needs --ssr)")
    ap.add_argument("--ssr-max-roughness", type=float, default=None, metavar="X", help="surfaces at or above this roughness do not reflect, 0 .. 1 (default 0.75; needs --ssr)")
    ap.add_argument("--ssr-gloss", action="store_true", help="experimental: the hit colour from a blurred pyramid of the lit frame, by the reflection cone (needs --ssr)")
    ap.add_argument("--ssr-cone", type=float, default=None, metavar="X", help="the cone's width per unit of roughness, 0 .. 16 (default 0: the sharp pass; needs --ssr-gloss)")
    ap.add_argument("--ssr-levels", type=int, default=None, metavar="N", help="levels of the pyramid, the frame counted, 1 .. 8 (default 6; needs --ssr-gloss)")
    ap.add_argument("--sky", action="store_true", help="render the procedural sky (a single-scattering atmosphere) under the sun of Lights[0] "
                    "into the cube map, with the chain, tail and table that --gloss, --env-ambient and --env-specular ask for")
    ap.add_argument("--sky-sun-elevation", type=float, default=None, metavar="DEG", help="the sun's elevation over the horizon, along the azimuth "
                    "of Lights[0] (default: where Lights[0] shines from; needs --sky)")
    ap.add_argument("--sky-steps", type=int, default=None, metavar="N", help="samples along each view ray, 1 .. 64 (default 16; needs --sky)")
    ap.add_argument("--fog", action="store_true", help="volumetric fog with sun shafts through the cascades, after the lighting pass")
    ap.add_argument("--fog-density", type=float, default=None, metavar="X", help="fog density, 0 .. 16 (default 0.02; needs --fog)")
    ap.add_argument("--fog-steps", type=int, default=None, metavar="N", help="samples along each view ray, 1 .. 64 (default 16; needs --fog)")
    ap.add_argument("--dof", action="store_true", help="depth of field from the depth plane, after the lighting pass and the fog")
    ap.add_argument("--dof-focus", type=float, default=None, metavar="X", help="view-space distance in focus (default 15; needs --dof)")
    ap.add_argument("--dof-aperture", type=float, default=None, metavar="X", help="circle-of-confusion radius in pixels of a point at infinity, "
                                                                                  "0 .. 64 (default 6; needs --dof)")
    ap.add_argument("--dof-radius", type=int, default=None, metavar="N", help="gather radius in pixels, 1 .. 8 (default 8; needs --dof)")
    ap.add_argument("--decals", action="store_true", help="a puddle on the floor and a mark on a box face, blended into the G-buffer")
    ap.add_argument("--bloom", action="store_true", help="bloom, after the lighting pass, the fog and the depth of field")
    ap.add_argument("--bloom-threshold", type=int, default=None, metavar="N", help="luma threshold, 0 .. 255 (default 192; needs --bloom)")
    ap.add_argument("--bloom-intensity", type=int, default=None, metavar="N", help="strength, 256 = 1.0, 0 .. 1024 (default 128; needs --bloom)")
    ap.add_argument("--bloom-levels", type=int, default=None, metavar="N", help="pyramid levels, 1 .. 8 (default 6; needs --bloom)")
    ap.add_argument("--taa", action="store_true", help="temporal anti-aliasing: jittered frames of the still scene blended into a history")
    ap.add_argument("--taa-upscale", default="", metavar="WxH", help="temporal upsampling: jittered frames of --size accumulated into a W x H history; "
                                                                     "the frame written has that size (not with --taa, --dof or --motion-blur)")
    ap.add_argument("--taa-frames", type=int, default=None, metavar="N", help="jittered frames to render (default 16; needs --taa or --taa-upscale)")
    ap.add_argument("--motion-blur", action="store_true", help="camera-motion blur, behind the depth of field and in front of the bloom")
    ap.add_argument("--motion-blur-shutter", type=int, default=None, metavar="N", help="exposure in 1/256 of the frame interval, 0 .. 256 (default 128; needs --motion-blur)")
    ap.add_argument("--motion-blur-samples", type=int, default=None, metavar="N", help="samples along the velocity: 2, 4, 8, 16 or 32 (default 8; needs --motion-blur)")
    ap.add_argument("--motion-blur-pan", type=float, default=None, metavar="DX", help="the previous camera's displacement along +x in world units (default 0.5; "
                                                                                      "needs --motion-blur)")
    ap.add_argument("--sharpen", action="store_true", help="contrast-adaptive sharpening behind the temporal stage, in front of --dof")
    ap.add_argument("--sharpen-strength", type=int, default=None, metavar="N", help="0 .. 256 (default: the pass's; needs --sharpen)")
    ap.add_argument("--grade-cube", default="", metavar="FILE.cube", help="colour grade through the 3D table of a .cube file, behind the bloom and in front of --aa")
    ap.add_argument("--grade-slope", default="", metavar="R,G,B", help="colour grade: the ASC CDL's slope, 0 .. 16 (default 1)")
    ap.add_argument("--grade-offset", default="", metavar="R,G,B", help="colour grade: the ASC CDL's offset, -4 .. 4 (default 0)")
    ap.add_argument("--grade-power", default="", metavar="R,G,B", help="colour grade: the ASC CDL's power, 1/16 .. 16 (default 1)")
    ap.add_argument("--grade-saturation", type=float, default=None, metavar="X", help="colour grade: saturation, 0 .. 4 (default 1)")
    a = ap.parse_args()
    grade = {}
    for name, text in (("slope", a.grade_slope), ("offset", a.grade_offset), ("power", a.grade_power)):
        if text:
            v = [float(x) for x in text.split(",")]
            if len(v) not in (1, 3):
                ap.error("--grade-%s takes R,G,B or one number" % name)
            grade[name] = v * 3 if len(v) == 1 else v
    if a.grade_saturation is not None:
        grade["saturation"] = a.grade_saturation
    if a.grade_cube and grade:
        ap.error("--grade-cube does not go with --grade-slope, --grade-offset, --grade-power or --grade-saturation")
    if a.sharpen_strength is not None and not a.sharpen:
        ap.error("--sharpen-strength needs --sharpen")
    if (a.motion_blur_shutter is not None or a.motion_blur_samples is not None or a.motion_blur_pan is not None) and not a.motion_blur:
        ap.error("--motion-blur-shutter, --motion-blur-samples and --motion-blur-pan need --motion-blur")
    if a.taa_frames is not None and not ((a.taa or a.taa_upscale) and a.taa_frames >= 1):
        ap.error("--taa-frames takes a positive count and needs --taa or --taa-upscale")
    if a.taa_upscale and (a.taa or a.dof or a.motion_blur):
        ap.error("--taa-upscale does not go with --taa, --dof or --motion-blur")
    if (a.bloom_threshold is not None or a.bloom_intensity is not None or a.bloom_levels is not None) and not a.bloom:
        ap.error("--bloom-threshold, --bloom-intensity and --bloom-levels need --bloom")
    if (a.dof_focus is not None or a.dof_aperture is not None or a.dof_radius is not None) and not a.dof:
        ap.error("--dof-focus, --dof-aperture and --dof-radius need --dof")
    if (a.fog_density is not None or a.fog_steps is not None) and not a.fog:
        ap.error("--fog-density and --fog-steps need --fog")
    ap_gloss = a.ssr_gloss or a.ssr_cone is not None or a.ssr_levels is not None
    if ap_gloss and not (a.ssr and a.ssr_gloss):
        ap.error("--ssr-gloss needs --ssr; --ssr-cone and --ssr-levels need --ssr-gloss")
    if (a.ssr_steps is not None or a.ssr_distance is not None or a.ssr_max_roughness is not None) and not a.ssr:
        ap.error("--ssr-steps, --ssr-distance and --ssr-max-roughness need --ssr")
    box = None
    if a.probe_box:
        if not (a.capture_env and a.gloss):
            ap.error("--probe-box needs --capture-env and --gloss")
        v = [float(x) for x in a.probe_box.split(",")]
        if len(v) != 6:
            ap.error("--probe-box takes X0,Y0,Z0,X1,Y1,Z1")
        box = (v[:3], v[3:])
    if a.env_specular and not a.gloss:
        ap.error("--env-specular needs --gloss")
    if a.gloss and not (a.cube or a.capture_env):
        ap.error("--gloss needs --cube or --capture-env")
    if a.env_ambient and not (a.cube or a.capture_env):
        ap.error("--env-ambient needs --cube or --capture-env")
    W, H = (int(v) for v in a.size.lower().split("x"))
    WO, HO = (int(v) for v in a.taa_upscale.lower().split("x")) if a.taa_upscale else (W, H)
    if not (W <= WO <= 4 * W and H <= HO <= 4 * H):
        ap.error("--taa-upscale takes a size whose sides are 1 to 4 times --size's")
    import torch
    from . import Context, Crychic, LIGHT_SKY, SceneGeometry, check, geometry as g, lib, scene
    from ._lib import BloomParams, DofParams, FogParams, MotionBlurParams, PassConstants, SsrParams
    ctx = Context(0)
    consts = scene.Constants(W, H, a.shadow_dim)
    tex = g.reference_textures(a.textures) if a.textures else g.procedural_textures(64)
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials(), tex)
    sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    cube = scene.make_cubemap(256, ctx.device)
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), cube, shadow_dim=a.shadow_dim, gbuffer_formats=a.gbuffer)
    if a.cube:            # with the mip chain the file stores, as the reference binds it (CRYCHIC.cpp:1148-1151)
        chain, dim, levels = g.load_dds_cube_mips(a.cube)
        chain = torch.from_numpy(chain).to(ctx.device)
        if a.gloss:
            if levels < 2:        # the file stores level 0 alone: its box chain, built on the device
                levels = g.cube_full_levels(dim)
                full = torch.empty((g.cube_chain_bytes(dim, levels),), dtype=torch.uint8, device=ctx.device)
                full[:chain.numel()] = chain
                chain = app.generate_cube_mips(full, dim, levels)
            chain = app.prefilter_cube_map(chain, dim, levels)
        if a.env_ambient or a.env_specular:
            if not a.gloss:
                levels = 1        # level 0 alone
            full = torch.empty(((g.cube_chain_env_bytes if a.env_specular else g.cube_chain_sh_bytes)(dim, levels),), dtype=torch.uint8,
                               device=ctx.device)
            full[:g.cube_chain_bytes(dim, levels)] = chain[:g.cube_chain_bytes(dim, levels)]
            chain = full
            if a.env_ambient:
                app.project_irradiance(chain, dim, levels)
            if a.env_specular:
                app.build_env_brdf(chain, dim, levels)
        app.set_cube_map(chain, dim=dim, levels=levels, gloss=a.gloss and levels > 1, ambient_sh=a.env_ambient, env_brdf=a.env_specular)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    for k in range(4):
        cb = PassConstants()
        cb.ViewProj[:] = list((consts.light_view[k].astype(np.float32) @ consts.light_proj[k].astype(np.float32)).T.reshape(-1))
        sgeo.DrawSceneToShadowMap(cb, app.mShadowMap.mShadowMap[k])
    def camera_passes():
        geo.DrawNormalsAndDepth(app.mMainPassCB, app.mSsao.mNormalMap, app.mDepthStencilBuffer)
        geo.DrawGBuffer(app.mMainPassCB, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
        if a.decals:
            app.apply_decals()
    geo.DrawNormalsAndDepth(app.mMainPassCB, app.mSsao.mNormalMap, app.mDepthStencilBuffer)
    geo.DrawGBuffer(app.mMainPassCB, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    if a.decals:          # once on each fresh G-buffer: a second application would stack
        from ._lib import DECAL_ALBEDO, DECAL_METALNESS, DECAL_NORMAL, DECAL_ROUGHNESS
        puddle = g.decal_from_box(g.decal_box_world((2.5, 0.0, -7.5), (1.5, 0.25, 1.5)), (64, 64), 0.5, 0.0, texture=0, normalTexture=1,
                                  flags=DECAL_ALBEDO | DECAL_ROUGHNESS | DECAL_NORMAL, roughness=0.03, opacity=0.85)
        mark = g.decal_from_box(g.decal_box_world((0.0, 0.8, -10.8), (0.6, 0.6, 0.3), down=False), (64, 64), 0.5, 0.0, texture=2,
                                flags=DECAL_ALBEDO | DECAL_METALNESS, metalness=0.0, tint=(0.9, 0.1, 0.1))
        app.set_decals([puddle, mark], [g.decal_texture("disc", 64), g.decal_texture("dent", 64), g.decal_texture("ring", 64)])
        app.apply_decals()
    app.blurCount, app.numDirLights, app.flags = 3, 1, LIGHT_SKY        # the reference's settings (CRYCHIC.cpp:221, Common.hlsl:6-8)
    if a.capture_env:
        pos = [float(v) for v in a.capture_env.split(",")]
        if len(pos) != 3:
            ap.error("--capture-env takes X,Y,Z")
        chain, dim, levels = app.capture_environment(pos, geo, sgeo, dim=a.capture_dim, prefilter=a.gloss, irradiance=a.env_ambient,
                                                     levels=1 if a.env_ambient and not a.gloss else None, env_brdf=a.env_specular, probe_box=box)
        app.set_cube_map(chain, dim, levels, gloss=a.gloss and levels > 1, ambient_sh=a.env_ambient, env_brdf=a.env_specular,
                         parallax=box is not None)
        print("captured the environment at (%g, %g, %g): %d-texel faces, %d levels" % (pos[0], pos[1], pos[2], dim, levels))
    if a.sky:
        from ._lib import SkyParams
        knobs = {} if a.sky_steps is None else dict(viewSteps=a.sky_steps)
        levels = None if a.gloss else 1
        if levels is None or a.env_ambient or a.env_specular:       # bind a cube map with the flags followSun is to keep
            chain, dim, levels = app.render_sky(SkyParams.default(**knobs), dim=256, levels=levels, prefilter=a.gloss, irradiance=a.env_ambient,
                                                env_brdf=a.env_specular)
            app.set_cube_map(chain, dim, levels, gloss=a.gloss and levels > 1, ambient_sh=a.env_ambient, env_brdf=a.env_specular)
        if a.sky_sun_elevation is None:
            app.followSun = SkyParams.default(**knobs) if knobs else True
            d = app.mMainPassCB.Lights[0].Direction
            sun = (-d[0], -d[1], -d[2])
        else:
            d = app.mMainPassCB.Lights[0].Direction
            az, el = math.atan2(-d[0], -d[2]), math.radians(a.sky_sun_elevation)
            sun = (math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az))
            chain, dim, levels = app.render_sky(SkyParams.default(sunDir=sun, **knobs), dim=256, levels=levels, prefilter=a.gloss,
                                                irradiance=a.env_ambient, env_brdf=a.env_specular)
            app.set_cube_map(chain, dim, levels, gloss=a.gloss and levels > 1, ambient_sh=a.env_ambient, env_brdf=a.env_specular)
        print("procedural sky: sun towards (%.3f, %.3f, %.3f), sun colour %s" % (sun + (tuple(round(c, 3) for c in app.sky_sun_colour(
            SkyParams.default(sunDir=sun, **knobs))),)))
    if a.ssr:
        knobs = {k: v for k, v in (("steps", a.ssr_steps), ("maxDistance", a.ssr_distance), ("maxRoughness", a.ssr_max_roughness)) if v is not None}
        app.ssr = SsrParams.default(**knobs) if knobs else True
        if a.ssr_gloss:
            from ._lib import SsrGlossParams
            knobs = {k: v for k, v in (("coneScale", a.ssr_cone), ("levels", a.ssr_levels)) if v is not None}
            app.ssrGloss = SsrGlossParams.default(**knobs) if knobs else True
    if a.fog:
        knobs = {k: v for k, v in (("density", a.fog_density), ("steps", a.fog_steps)) if v is not None}
        app.fog = FogParams.default(**knobs) if knobs else True
    if a.dof:
        app.depthOfField = DofParams.default(focus=a.dof_focus, aperture=a.dof_aperture, radius=a.dof_radius)
    if a.bloom:
        app.bloom = BloomParams.default(threshold=a.bloom_threshold, intensity=a.bloom_intensity, levels=a.bloom_levels)
    if a.sharpen:
        from ._lib import SharpenParams
        app.sharpening = SharpenParams.default(strength=a.sharpen_strength)
    if a.grade_cube:
        app.colourGrade = a.grade_cube
    elif grade:
        from ._lib import GradeParams
        app.colourGrade = GradeParams.default(**grade)
    if a.aa:
        app.antiAliasing = True
    prev_view_proj = None
    if a.motion_blur:
        app.motionBlur = MotionBlurParams.default(shutter=a.motion_blur_shutter, samples=a.motion_blur_samples)
        before = scene.default_camera(W, H)
        before.pos[0] += 0.5 if a.motion_blur_pan is None else a.motion_blur_pan
        prev_view_proj = scene.Constants(W, H, a.shadow_dim, cam=before).pass_cb.ViewProj
    if a.taa or a.taa_upscale:
        # the still scene under the jitter sequence: the camera planes are rasterised again with each frame's shifted projection, the
        # pass gets the unjittered ViewProj of the same camera for this frame and the previous one
        if a.taa:
            app.temporalAA = True
        else:
            app.temporalUpscale = (WO, HO)
        jx, jy = C.c_float(), C.c_float()
        frames = a.taa_frames or 16
        for k in range(frames):
            check(lib.crychic_taa_jitter(k, C.byref(jx), C.byref(jy)))
            jittered = scene.Constants(W, H, a.shadow_dim, jitter=(jx.value, jy.value))
            app.mMainPassCB, app.mSsaoCB = jittered.pass_cb, jittered.ssao_cb
            camera_passes()
            if prev_view_proj is not None and k == frames - 1:
                app.set_frame_view_proj(prev_view_proj)
            app.set_frame_view_proj(consts.pass_cb.ViewProj, jitter=(jx.value, jy.value))
            app.Draw()
    else:
        if prev_view_proj is not None:
            app.set_frame_view_proj(prev_view_proj)
            app.set_frame_view_proj(consts.pass_cb.ViewProj)
        app.Draw()
    torch.cuda.synchronize()
    img = np.ascontiguousarray(app.final_frame().cpu().numpy())
    check(lib.crychic_save_ppm(a.out.encode(), img.ctypes.data, WO, HO))
    chain = (("ssr", "screen-space reflections"), ("fog", "fog"), ("temporalAA", "temporal anti-aliasing"), ("temporalUpscale", "temporal upsampling"), ("sharpening", "sharpened"), ("depthOfField", "depth of field"), ("motionBlur", "motion blur"),
             ("bloom", "bloom"), ("colourGrade", "colour grade"), ("antiAliasing", "anti-aliased"))                   # Draw()'s order
    print("wrote %s (%dx%d%s) on %s" % (a.out, WO, HO, "".join(", " + text for switch, text in chain if getattr(app, switch) is not None and getattr(app, switch) is not False),
                                        ctx.device_name))


if __name__ == "__main__":
    main()
