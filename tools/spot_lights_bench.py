"""Timing of the spot-light extension (include/crychic_hip.h crychic_deferred_light_spots); prints one JSON line.

    python tools/spot_lights_bench.py [--steps 50] [--warmup 5]

Per leg: the median HIP-event time of the lighting pass (light_ms) and of the whole hot path (total_ms, SSAO + blur + lighting)
over --steps frames, from the context's per-pass events (crychic_ctx_set_profiling).  Legs:
  4k_none / 4k_spots32         3840 x 2160, reference camera, no local lights / 32 spot lights (scene.spot_light_ring)
  8k_points64_spots64          7680 x 4320, the 8 x 8 point grid plus a ring of 64 spot lights
  8k_points64 / 8k_spots64_p0  7680 x 4320, the 8 x 8 point grid as point lights / as spot lights with SpotPower 0 at the same
                               positions (the same bits: `p0_same_bits`), timed in alternating rounds; `p0_over_points` is the
                               ratio of their lighting-pass medians.
The scene, blur count (4), directional lights (3) and literal PCF radius are bench.py's defaults.  Needs a HIP device."""
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
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds of the SpotPower-0 / point-light comparison")
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, scene
    from crychic_renderer_amd._lib import lib
    if not torch.cuda.is_available():
        sys.exit("spot_lights_bench.py needs a HIP device")
    ctx = Context(0)
    SD, CD = 4096, 256
    radius = lib.crychic_pcf_search_radius(SD, 1)

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

    def leg(light, total):
        return {"light_ms": round(statistics.median(light), 4), "total_ms": round(statistics.median(total), 4), "frames": len(light)}

    legs = {}
    app = make_app(3840, 2160)
    legs["4k_none"] = leg(*timed(app, args.steps))
    app.set_spot_lights(scene.spot_light_ring(32))
    legs["4k_spots32"] = leg(*timed(app, args.steps))
    del app
    torch.cuda.empty_cache()

    app = make_app(7680, 4320)
    grid = scene.point_light_grid(8)
    app.set_point_lights(grid)
    app.set_spot_lights(scene.spot_light_ring(64))
    legs["8k_points64_spots64"] = leg(*timed(app, args.steps))
    grid0 = scene.point_light_grid(8)
    for k in range(len(grid0)):
        grid0[k].SpotPower = 0.0
    frames, acc = {}, {"8k_points64": ([], []), "8k_spots64_p0": ([], [])}
    per_round = max(1, args.steps // args.rounds)
    for _ in range(args.rounds):
        for name, points, spots in (("8k_points64", grid, None), ("8k_spots64_p0", None, grid0)):
            app.set_point_lights(points)
            app.set_spot_lights(spots)
            light, total = timed(app, per_round)
            acc[name][0].extend(light)
            acc[name][1].extend(total)
            torch.cuda.synchronize()
            frames[name] = app.mBackBuffer.clone()
    for name, (light, total) in acc.items():
        legs[name] = leg(light, total)
    same = bool(torch.equal(frames["8k_points64"], frames["8k_spots64_p0"]))
    out = {"metric": "spot_lights_light_ms", "device": ctx.device_name, "legs": legs, "p0_same_bits": same,
           "p0_over_points": round(legs["8k_spots64_p0"]["light_ms"] / legs["8k_points64"]["light_ms"], 4)}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
