"""Timing of the environment BRDF table build and of the lighting pass with the split-sum reflection weight;
prints one JSON line.

    python tools/env_brdf_bench.py [--steps 50] [--warmup 5] [--out profiles/env_brdf_bench.json]

Legs, each the median of HIP-event times over --steps runs (torch events on the caller's stream, around work that is synchronised):
  build      crychic_build_env_brdf (one launch, 1024 wavefronts): us.
  light_4k   the lighting pass (the library's events around it: last_pass_times()["light_ms"]) of the 3840 x 2160 frame of
             scene.make_scene (blurCount 4, 3 directional lights, 256-texel cube map) over the prefiltered 9-level chain in four
             variants alternated frame by frame: CRYCHIC_LIGHT_CUBE_LEVELS(9) | CRYCHIC_LIGHT_CUBE_GLOSS; the same with
             CRYCHIC_LIGHT_ENV_BRDF; both again with CRYCHIC_LIGHT_AMBIENT_SH.
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
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, geometry as g, scene
    if not torch.cuda.is_available():
        sys.exit("env_brdf_bench.py needs a HIP device")
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
    box, nlev = g.cube_mip_chain(planes["cube"].cpu().numpy())
    box = torch.from_numpy(box).to(ctx.device)
    chain = torch.zeros((g.cube_chain_env_bytes(256, nlev),), dtype=torch.uint8, device=ctx.device)
    app.prefilter_cube_map(box, 256, nlev, out=chain)
    app.project_irradiance(chain, 256, nlev)

    # ---- the table build alone
    for _ in range(args.warmup):
        app.build_env_brdf(chain, 256, nlev)
    t = [event_ms(lambda: app.build_env_brdf(chain, 256, nlev)) for _ in range(args.steps)]
    legs["build"] = {"texels": 1024, "samples_per_texel": 4096, "launches": 1, "build_us": round(med(t) * 1e3, 2),
                     "build_us_min_max": [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)], "runs": args.steps}

    # ---- the 4K lighting pass over the gloss chain: without and with the flag, and the same with SH
    variants = {"gloss": new_app(), "gloss_spec": new_app(), "gloss_sh": new_app(), "gloss_sh_spec": new_app()}
    variants["gloss"].set_cube_map(chain, dim=256, levels=nlev, gloss=True)
    variants["gloss_spec"].set_cube_map(chain, dim=256, levels=nlev, gloss=True, env_brdf=True)
    variants["gloss_sh"].set_cube_map(chain, dim=256, levels=nlev, gloss=True, ambient_sh=True)
    variants["gloss_sh_spec"].set_cube_map(chain, dim=256, levels=nlev, gloss=True, ambient_sh=True, env_brdf=True)
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
    legs["light_4k"]["gloss_spec_over_gloss"] = round(med(times["gloss_spec"]) / med(times["gloss"]), 4)
    legs["light_4k"]["gloss_sh_spec_over_gloss_sh"] = round(med(times["gloss_sh_spec"]) / med(times["gloss_sh"]), 4)
    line = json.dumps({"metric": "env_brdf", "device": name, "legs": legs})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
