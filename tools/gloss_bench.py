"""Timing of the roughness prefilter and of the glossy reflection lookup; prints one JSON line.

    python tools/gloss_bench.py [--steps 50] [--warmup 5] [--out profiles/gloss_bench.json]

Legs, each the median of HIP-event times over --steps runs (torch events on the caller's stream, around work that is synchronised):
  prefilter_dim256 / prefilter_dim1024   crychic_prefilter_cube_chain of a noise cube's box chain, full chain (9 / 11 levels): us, and
                                         the texel lookups (output texels x kept samples x 2 levels x 4 texels) per second.
  capture_dim256                         Crychic.capture_environment of the box-and-grid scene at (2.5, 1.25, 2.5), shadow_dim 1024, into
                                         a kept buffer, without and with prefilter=True, alternated run by run: both totals and the ratio.
  light_4k                               the lighting pass (the library's events around it: last_pass_times()["light_ms"]) of the
                                         3840 x 2160 frame of scene.make_scene (blurCount 4, 3 directional lights, 256-texel cube map)
                                         in three variants alternated frame by frame: level 0; CRYCHIC_LIGHT_CUBE_LEVELS(9) with the box
                                         chain (bench.py's cube_mip_chain leg); the same with CRYCHIC_LIGHT_CUBE_GLOSS over the
                                         prefiltered chain.
Needs a HIP device."""
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
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, SceneGeometry, geometry as g, scene
    if not torch.cuda.is_available():
        sys.exit("gloss_bench.py needs a HIP device")
    ctx = Context(0)
    name = ctx.device_name
    med = statistics.median

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    legs = {}
    W, H = 3840, 2160
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))

    def new_app():
        a = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
        a.load_scene(planes)
        a.blurCount, a.numDirLights, a.flags = 4, 3, LIGHT_SKY
        return a

    app = new_app()
    # ---- the prefilter alone
    for dim in (256, 1024):
        cube = np.random.default_rng(dim).integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)
        levels = g.cube_full_levels(dim)
        box = torch.zeros((g.cube_chain_bytes(dim, levels),), dtype=torch.uint8, device=ctx.device)
        box[:cube.size] = torch.from_numpy(cube.reshape(-1)).to(ctx.device)
        app.generate_cube_mips(box, dim, levels)
        out = torch.empty_like(box)
        for _ in range(args.warmup):
            app.prefilter_cube_map(box, dim, levels, out=out)
        t = [event_ms(lambda: app.prefilter_cube_map(box, dim, levels, out=out)) for _ in range(args.steps)]
        lookups = sum(6 * max(dim >> k, 1) ** 2 * len(g.cube_prefilter_samples(dim, levels, k)[0]) * 8 for k in range(1, levels))
        legs["prefilter_dim%d" % dim] = {"levels": levels, "launches": levels - 1, "prefilter_us": round(med(t) * 1e3, 2),
                                         "texel_lookups": lookups, "glookups_per_s": round(lookups / (med(t) * 1e-3) / 1e9, 2), "runs": args.steps}
        del box, out

    # ---- a capture without and with the prefilter, alternated
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials(), g.procedural_textures(64))
    sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    pos, SD, dim = (2.5, 1.25, 2.5), 1024, 256
    out = torch.empty((g.cube_chain_bytes(dim, g.cube_full_levels(dim)),), dtype=torch.uint8, device=ctx.device)
    capture = lambda pre: app.capture_environment(pos, geo, sgeo, dim=dim, shadow_dim=SD, out=out, prefilter=pre)
    for _ in range(args.warmup):
        capture(False); capture(True)
    plain, pre = [], []
    for _ in range(args.steps):
        plain.append(event_ms(lambda: capture(False)))
        pre.append(event_ms(lambda: capture(True)))
    legs["capture_dim256"] = {"shadow_dim": SD, "capture_ms": round(med(plain), 4), "capture_prefilter_ms": round(med(pre), 4),
                              "prefilter_over_capture": round(med(pre) / med(plain), 4), "runs": args.steps}

    # ---- the 4K lighting pass: level 0, the box chain by derivatives, the prefiltered chain by roughness
    box, nlev = g.cube_mip_chain(planes["cube"].cpu().numpy())
    box = torch.from_numpy(box).to(ctx.device)
    gloss = app.prefilter_cube_map(box, 256, nlev)
    variants = {"level0": new_app(), "cube_levels": new_app(), "cube_levels_gloss": new_app()}
    variants["cube_levels"].set_cube_map(box, dim=256, levels=nlev)
    variants["cube_levels_gloss"].set_cube_map(gloss, dim=256, levels=nlev, gloss=True)
    times = {k: [] for k in variants}
    for a in variants.values():
        a.set_profiling(True)
        for _ in range(args.warmup):
            a.Draw()
    torch.cuda.synchronize()
    for _ in range(args.steps):
        for k, a in variants.items():
            a.Draw()
            times[k].append(a.last_pass_times()["light_ms"])
    legs["light_4k"] = dict({"cube_levels": nlev, "runs": args.steps},
                            **{k + "_light_ms": round(med(v), 4) for k, v in times.items()},
                            **{k + "_light_ms_min_max": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
    legs["light_4k"]["gloss_over_cube_levels"] = round(med(times["cube_levels_gloss"]) / med(times["cube_levels"]), 4)
    line = json.dumps({"metric": "gloss", "device": name, "legs": legs})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
