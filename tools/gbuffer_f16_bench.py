"""Timing of the G-buffer plane formats (include/crychic_hip.h CRYCHIC_GBUFFER_G*_F16); prints one JSON line.

    python tools/gbuffer_f16_bench.py [--steps 48] [--warmup 5] [--rounds 4]

One process, legs alternated in --rounds rounds, median HIP-event times.  Formats: f32 = three float4 planes (48 B per pixel),
mixed = G0 float4 with G1 and G2 half4 (32 B), f16 = all three half4 (24 B).  Legs:
  4k_ref_<fmt> / 4k_covered_<fmt>   3840 x 2160, reference camera / covered camera (no sky pixel: every G-buffer texel is read)
  8k_points64_<fmt>                 7680 x 4320, reference camera, the 8 x 8 point-light grid
Per leg: light_ms and total_ms (SSAO + blur + lighting) from the context's per-pass events, producer_ms (the fused normals + depth +
G-buffer pass of the reference scene into planes of the leg's formats, torch events), gbuffer_MB, and hbm_roofline_frac: SURVEY.md
8d's algorithmic bytes of the frame, (59 + 14 blurCount) N with the 16 N of each half4 plane replaced by 8 N, over total_ms and
the HBM peak.  light_vs_f32 / total_vs_f32 / producer_vs_f32 compare a leg with the f32 leg of the same camera in the same run.
The scene, blur count (4), directional lights (3) and literal PCF radius are bench.py's defaults.  Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X, as bench.py
FORMATS = ("f32", "mixed", "f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--skip-8k", action="store_true")
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, SceneGeometry, geometry as g, gbuffer_formats, scene
    from crychic_renderer_amd._lib import lib
    if not torch.cuda.is_available():
        sys.exit("gbuffer_f16_bench.py needs a HIP device")
    ctx = Context(0)
    SD, CD, BC = 4096, 256, 4
    radius = lib.crychic_pcf_search_radius(SD, 1)
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials(), g.procedural_textures(64))

    def make_app(W, H, fmt, covered, points):
        consts = scene.Constants(W, H, SD, cam=scene.covered_camera(W, H)) if covered else None
        planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=CD, device=str(ctx.device), consts=consts)
        app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD, gbuffer_formats=fmt)
        app.load_scene(planes)              # the fp32 planes converted to the leg's formats
        app.blurCount, app.numDirLights, app.pcfSearchRadius = BC, 3, radius
        if points:
            app.set_point_lights(scene.point_light_grid(8))
        # the producer pass writes planes of its own (same formats), so the lighting legs keep the planes every format shares
        dt = {"f32": torch.float32, "f16": torch.float16}
        scratch = {"g": [torch.zeros((H, W, 4), dtype=dt[f], device=ctx.device) for f in gbuffer_formats(fmt)],
                   "normal": torch.zeros((H, W, 4), dtype=torch.float16, device=ctx.device),
                   "depth": torch.zeros((H, W), dtype=torch.int32, device=ctx.device)}
        return app, scratch

    def timed(app, scratch, steps, acc):
        for _ in range(args.warmup):
            app.Draw()
        app.set_profiling(True)
        for _ in range(steps):
            app.Draw()
            t = app.last_pass_times()
            acc["light"].append(t["light_ms"])
            acc["total"].append(t["total_ms"])
        app.set_profiling(False)
        for k in range(2 + steps // 4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            geo.DrawNormalsDepthAndGBuffer(app.mMainPassCB, scratch["normal"], scratch["g"], scratch["depth"])
            e1.record()
            e1.synchronize()
            if k >= 2:
                acc["producer"].append(e0.elapsed_time(e1))

    def run_group(W, H, specs):
        """specs: [(leg name, fmt, covered, points)] -- built together, timed in alternating rounds."""
        apps = {name: make_app(W, H, fmt, covered, points) for name, fmt, covered, points in specs}
        acc = {name: {"light": [], "total": [], "producer": []} for name in apps}
        per_round = max(1, args.steps // args.rounds)
        for _ in range(args.rounds):
            for name, (app, scratch) in apps.items():
                timed(app, scratch, per_round, acc[name])
        out = {}
        npx = W * H
        for name, fmt, covered, points in specs:
            a = acc[name]
            halves = sum(f == "f16" for f in gbuffer_formats(fmt))
            frame_bytes = (59 + 14 * BC - 8 * halves) * npx
            total = statistics.median(a["total"])
            out[name] = {"light_ms": round(statistics.median(a["light"]), 4), "total_ms": round(total, 4),
                         "producer_ms": round(statistics.median(a["producer"]), 4), "frames": len(a["light"]),
                         "gbuffer_MB": round((48 - 8 * halves) * npx / 1e6, 1), "frame_algorithmic_MB": round(frame_bytes / 1e6, 1),
                         "hbm_roofline_frac": round(frame_bytes / (total * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        for name, fmt, covered, points in specs:
            base = out[name.rsplit("_", 1)[0] + "_f32"]
            for k in ("light", "total", "producer"):
                out[name][k + "_vs_f32"] = round(out[name][k + "_ms"] / base[k + "_ms"], 4)
        del apps
        torch.cuda.empty_cache()
        return out

    legs = {}
    legs.update(run_group(3840, 2160, [("4k_%s_%s" % (cam, f), f, cam == "covered", False) for cam in ("ref", "covered") for f in FORMATS]))
    if not args.skip_8k:
        legs.update(run_group(7680, 4320, [("8k_points64_%s" % f, f, False, True) for f in FORMATS]))
    print(json.dumps({"metric": "gbuffer_formats_ms", "device": ctx.device_name, "blur_count": BC, "legs": legs}))
    ctx.close()


if __name__ == "__main__":
    main()
