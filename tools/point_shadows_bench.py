"""Timing of the shadowed point lights (include/crychic_hip.h crychic_deferred_light_point_shadows); prints one JSON line.

    python tools/point_shadows_bench.py [--steps 50] [--warmup 5]

3840 x 2160 and 7680 x 4320 frames of scene.make_scene with the 8 x 8 point grid (scene.point_light_grid(8), BASELINE configs[4]'s
lights).  Per frame size, legs with 0 and with 4 shadowed point lights (the first four of the grid) at face sizes 512 and 1024:
light_ms / total_ms are the median HIP-event times of the lighting pass and the hot path over --steps frames
(crychic_ctx_set_profiling), with faces the rasteriser rendered from the reference scene beforehand; producer_ms is the median time
of DrawPointShadowMaps, the 24 faces in two crychic_draw_scene_to_shadow_maps calls (torch events).  `shadow4_over_none` is the
lighting-pass ratio.  Blur count (4), directional lights (3) and literal PCF radius are bench.py's defaults.  Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, SceneGeometry, geometry as g, scene
    from crychic_renderer_amd._lib import lib
    if not torch.cuda.is_available():
        sys.exit("point_shadows_bench.py needs a HIP device")
    ctx = Context(0)
    SD, CD = 4096, 256
    radius = lib.crychic_pcf_search_radius(SD, 1)
    sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))

    def make_app(W, H):
        planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=CD, device=str(ctx.device))
        app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD)
        app.load_scene(planes)
        app.blurCount, app.numDirLights, app.pcfSearchRadius = 4, 3, radius
        return app

    def timed(app, steps):
        for _ in range(args.warmup):
            app.Draw()
        app.set_profiling(True)
        light, total = [], []
        for _ in range(steps):
            app.Draw()
            t = app.last_pass_times()
            light.append(t["light_ms"])
            total.append(t["total_ms"])
        app.set_profiling(False)
        return light, total

    def producer(app, steps):
        for _ in range(args.warmup):
            app.DrawPointShadowMaps(sgeo)
        times = []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            app.DrawPointShadowMaps(sgeo)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        return round(statistics.median(times), 4)

    def leg(light, total):
        return {"light_ms": round(statistics.median(light), 4), "total_ms": round(statistics.median(total), 4), "frames": len(light)}

    legs = {}
    for tag, W, H in (("4k", 3840, 2160), ("8k", 7680, 4320)):
        app = make_app(W, H)
        app.set_point_lights(scene.point_light_grid(8))
        legs[tag + "_shadow0"] = leg(*timed(app, args.steps))
        for dim in (512, 1024):
            app.set_point_shadows(4, dim=dim)
            prod = producer(app, args.steps)
            torch.cuda.synchronize()
            lit = float((app.mPointShadowMaps < 0xFFFFFF).float().mean())
            key = "%s_shadow4_dim%d" % (tag, dim)
            legs[key] = dict(leg(*timed(app, args.steps)), producer24_ms=prod, face_coverage=round(lit, 3))
            legs[key]["shadow4_over_none"] = round(legs[key]["light_ms"] / legs[tag + "_shadow0"]["light_ms"], 4)
            app.set_point_shadows(0)
        del app
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "point_shadows_light_ms", "device": ctx.device_name, "legs": legs}))
    ctx.close()


if __name__ == "__main__":
    main()
