"""Cost of the procedural sky; prints one JSON line.

    python tools/sky_bench.py [--steps 50] [--warmup 5] [--out profiles/sky_bench.txt]

Timed with HIP events on the context's stream after --warmup untimed rounds, the median of --steps rounds each:
  (a) launch_us[dim][steps]   crychic_render_sky of all six faces alone, at dim 64, 256 and 1024, at the default step counts and at
      64 x 32, each as 10 calls back to back between one pair of events (per call, without the gap an event pair adds);
  (b) chain_ms                Crychic.render_sky(dim=256, prefilter=True, irradiance=True): level 0, the mips, the SH projection and
      the prefilter;
  (c) capture_ms              one Crychic.capture_environment at the same dim with no geometry (six sky frames of the hot path, then
      the mips): what a sky cost before, given a cube map to capture from;
  (d) draw_4k_ms              the lighting frame of bench.py's scene (3840 x 2160, blurCount 4, 3 lights, sky), for scale.
valu_bound_us is the time the kernel's VALU instruction count per texel (read off the ISA, VALU_* below) implies at one wave64
VALU instruction per SIMD per two cycles (gfx950's SIMDs are 32 lanes wide) on 1024 SIMDs at 2.4 GHz; no counter was read for it.  Outputs are compared with nothing
here: tests/test_sky_gpu.py does that.  Needs a HIP device."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# VALU instructions of sky_kernel per lane, counted in the gfx950 ISA (hipcc -O3 -save-temps): the inner loop's body per sun sample,
# the rest of the outer loop's body per view sample, and everything outside the loops on the path of a lit texel of the sky
VALU_SUN_SAMPLE, VALU_VIEW_SAMPLE, VALU_FIXED = 47, 129, 250
SIMDS, HZ, CYCLES_PER_VALU = 1024, 2.4e9, 2


def valu_per_texel(view, sun):
    return view * (sun * VALU_SUN_SAMPLE + VALU_VIEW_SAMPLE) + VALU_FIXED


def valu_bound_us(dim, view, sun):
    waves = 6 * dim * dim / 64.0
    return 1e6 * waves * valu_per_texel(view, sun) * CYCLES_PER_VALU / (SIMDS * HZ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, SkyParams, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("sky_bench.py needs a HIP device")
    ctx = Context(0)
    W, H = 3840, 2160
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 4, 3, LIGHT_SKY
    stream = torch.cuda.current_stream(ctx.device)
    cube = torch.empty((6 * 1024 * 1024 * 4,), dtype=torch.uint8, device=ctx.device)
    default = SkyParams.default()
    fine = SkyParams.default(viewSteps=64, sunSteps=32)

    def launch(dim, p):
        def fn():
            check(lib.crychic_render_sky(ctx.handle, C.c_void_p(cube.data_ptr()), dim, 0, 6, C.byref(p), C.c_void_p(stream.cuda_stream)))
        return fn

    chain_out = torch.empty((app.render_sky(dim=256, prefilter=True, irradiance=True)[0].numel(),), dtype=torch.uint8, device=ctx.device)
    capture_out = torch.empty((chain_out.numel(),), dtype=torch.uint8, device=ctx.device)

    def timed(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n          # ms per call

    legs = {}
    for dim in (64, 256, 1024):
        legs["launch_%d_default" % dim] = (launch(dim, default), 10)
        legs["launch_%d_64x32" % dim] = (launch(dim, fine), 10 if dim < 1024 else 2)
    legs["chain"] = (lambda: app.render_sky(dim=256, prefilter=True, irradiance=True, out=chain_out), 1)
    legs["capture"] = (lambda: app.capture_environment((0.0, 2.0, 0.0), None, dim=256, out=capture_out), 1)
    legs["draw_4k"] = (app.Draw, 1)
    for _ in range(args.warmup):
        for fn, _n in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, (fn, n) in legs.items():
            times[k].append(timed(fn, n))
    med = statistics.median
    out = {"metric": "sky", "device": ctx.device_name, "runs": args.steps, "default_steps": [default.viewSteps, default.sunSteps]}
    for dim in (64, 256, 1024):
        for tag, (v, s) in (("default", (default.viewSteps, default.sunSteps)), ("64x32", (64, 32))):
            k = "launch_%d_%s" % (dim, tag)
            us, bound = 1e3 * med(times[k]), valu_bound_us(dim, v, s)
            out[k + "_us"] = round(us, 2)
            out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
            out[k + "_valu_bound_us"] = round(bound, 2)
            out[k + "_share_of_bound"] = round(bound / us, 3)
    out["valu_per_texel"] = {"default": valu_per_texel(default.viewSteps, default.sunSteps), "64x32": valu_per_texel(64, 32)}
    out["chain_ms"] = round(med(times["chain"]), 4)
    out["capture_ms"] = round(med(times["capture"]), 4)
    out["draw_4k_ms"] = round(med(times["draw_4k"]), 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
