"""Timing of the SH9 irradiance projection and of the lighting pass with the ambient term from it; prints one
JSON line.

    python tools/env_ambient_bench.py [--steps 50] [--warmup 5] [--out profiles/env_ambient_bench.json]

Legs, each the median of HIP-event times over --steps runs (torch events on the caller's stream, around work that is synchronised):
  project_dim256 / project_dim1024   crychic_project_cube_sh of a noise level (three launches): us.
  capture_dim256                     Crychic.capture_environment of the box-and-grid scene at (2.5, 1.25, 2.5), shadow_dim 1024, into a
                                     kept buffer with prefilter=True, without and with irradiance=True, alternated run by run.
  light_4k                           the lighting pass (the library's events around it: last_pass_times()["light_ms"]) of the
                                     3840 x 2160 frame of scene.make_scene (blurCount 4, 3 directional lights, 256-texel cube map) in
                                     four variants alternated frame by frame: level 0; level 0 with CRYCHIC_LIGHT_AMBIENT_SH;
                                     CRYCHIC_LIGHT_CUBE_LEVELS(9) | CRYCHIC_LIGHT_CUBE_GLOSS over the prefiltered chain; the same with
                                     the flag.
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
        sys.exit("env_ambient_bench.py needs a HIP device")
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
    # ---- the projection alone
    for dim in (256, 1024):
        cube = np.random.default_rng(dim).integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)
        buf = torch.zeros((g.cube_chain_sh_bytes(dim, 1),), dtype=torch.uint8, device=ctx.device)
        buf[:cube.size] = torch.from_numpy(cube.reshape(-1)).to(ctx.device)
        for _ in range(args.warmup):
            app.project_irradiance(buf, dim, 1)
        t = [event_ms(lambda: app.project_irradiance(buf, dim, 1)) for _ in range(args.steps)]
        legs["project_dim%d" % dim] = {"texels": 6 * dim * dim, "launches": 3, "project_us": round(med(t) * 1e3, 2),
                                       "project_us_min_max": [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)], "runs": args.steps}
        del buf

    # ---- a capture without and with the projection, alternated
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials(), g.procedural_textures(64))
    sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    pos, SD, dim = (2.5, 1.25, 2.5), 1024, 256
    out = torch.empty((g.cube_chain_sh_bytes(dim, g.cube_full_levels(dim)),), dtype=torch.uint8, device=ctx.device)
    capture = lambda sh: app.capture_environment(pos, geo, sgeo, dim=dim, shadow_dim=SD, out=out, prefilter=True, irradiance=sh)
    for _ in range(args.warmup):
        capture(False); capture(True)
    plain, sh = [], []
    for _ in range(args.steps):
        plain.append(event_ms(lambda: capture(False)))
        sh.append(event_ms(lambda: capture(True)))
    legs["capture_dim256"] = {"shadow_dim": SD, "capture_prefilter_ms": round(med(plain), 4), "capture_prefilter_irradiance_ms": round(med(sh), 4),
                              "irradiance_over_capture": round(med(sh) / med(plain), 4), "runs": args.steps}

    # ---- the 4K lighting pass: level 0 and the gloss chain, each without and with the flag
    box, nlev = g.cube_mip_chain(planes["cube"].cpu().numpy())
    box = torch.from_numpy(box).to(ctx.device)
    gloss = torch.zeros((g.cube_chain_sh_bytes(256, nlev),), dtype=torch.uint8, device=ctx.device)
    app.prefilter_cube_map(box, 256, nlev, out=gloss)
    app.project_irradiance(gloss, 256, nlev)
    level0 = torch.zeros((g.cube_chain_sh_bytes(256, 1),), dtype=torch.uint8, device=ctx.device)
    level0[:6 * 256 * 256 * 4] = planes["cube"].reshape(-1)
    app.project_irradiance(level0, 256, 1)
    variants = {"level0": new_app(), "level0_sh": new_app(), "gloss": new_app(), "gloss_sh": new_app()}
    variants["level0"].set_cube_map(level0, dim=256, levels=1)
    variants["level0_sh"].set_cube_map(level0, dim=256, levels=1, ambient_sh=True)
    variants["gloss"].set_cube_map(gloss, dim=256, levels=nlev, gloss=True)
    variants["gloss_sh"].set_cube_map(gloss, dim=256, levels=nlev, gloss=True, ambient_sh=True)
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
    legs["light_4k"]["level0_sh_over_level0"] = round(med(times["level0_sh"]) / med(times["level0"]), 4)
    legs["light_4k"]["gloss_sh_over_gloss"] = round(med(times["gloss_sh"]) / med(times["gloss"]), 4)
    line = json.dumps({"metric": "env_ambient", "device": name, "legs": legs})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
