"""Cost of the box-projected reflection lookup on the 4K lighting pass; prints one JSON line.

    python tools/parallax_bench.py [--steps 50] [--warmup 5] [--out profiles/parallax_ab.txt]

The lighting pass (the library's events around it: last_pass_times()["light_ms"]) of the 3840 x 2160 frame of scene.make_scene
(blurCount 4, 3 directional lights, 256-texel cube map) over the prefiltered 9-level chain with CRYCHIC_LIGHT_CUBE_GLOSS |
CRYCHIC_LIGHT_ENV_BRDF | CRYCHIC_LIGHT_AMBIENT_SH, without and with CRYCHIC_LIGHT_CUBE_PARALLAX, on the same frame, alternated frame by
frame in one process: the median of --steps frames each.  The probe volume holds the whole scene.  Needs a HIP device."""
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
        sys.exit("parallax_bench.py needs a HIP device")
    ctx = Context(0)
    med = statistics.median
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
    app.build_env_brdf(chain, 256, nlev)
    volume = ((0.0, 3.0, 0.0), (-60.0, -1.0, -60.0), (60.0, 40.0, 60.0))
    app.set_probe_volume(chain, 256, nlev, *volume)
    variants = {"distant": new_app(), "box": new_app()}
    variants["distant"].set_cube_map(chain, dim=256, levels=nlev, gloss=True, ambient_sh=True, env_brdf=True)
    variants["box"].set_cube_map(chain, dim=256, levels=nlev, gloss=True, ambient_sh=True, env_brdf=True, parallax=True)
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
    differs = bool((variants["distant"].mBackBuffer != variants["box"].mBackBuffer).any().item())
    leg = dict({"cube_levels": nlev, "runs": args.steps, "probe_volume": volume, "frames_differ": differs},
               **{k + "_light_ms": round(med(v), 4) for k, v in times.items()},
               **{k + "_light_ms_min_max": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
    leg["box_over_distant"] = round(med(times["box"]) / med(times["distant"]), 4)
    line = json.dumps({"metric": "parallax", "device": ctx.device_name, "legs": {"light_4k_gloss_sh_spec": leg}})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
