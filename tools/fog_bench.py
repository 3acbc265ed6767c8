"""Cost of the volumetric fog pass on the benchmark's 4K frame; prints one JSON line.

    python tools/fog_bench.py [--steps 200] [--warmup 10] [--out profiles/fog_bench.txt]

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map, four
4096 x 4096 cascades), lit once; then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round
by round in one process, the median of --steps rounds each:
  (a) fog_n8_us .. fog_n64_us   crychic_fog of that frame alone (out of place) at N = 8, 16, 32, 64 steps, the other parameters default;
  (b) memcpy_us                 hipMemcpyAsync, device to device, of the same 33.2 MB plane -- the yardstick for "read twice, write once";
  (c) light_us                  crychic_deferred_light of the same frame -- the yardstick for a gather-bound full-screen pass;
  (d) fog_density0_us           (a) at N = 16 with density 0: every wavefront takes the copy exit -- the streaming skeleton;
  (e) draw_ms / draw_fog_ms     Crychic.Draw() without and with fog set (the defaults, N = 16).
gather_ns_n*: ((a) - (d)) / (W H N), the cost of one step of one pixel.  The output of (a) is compared with nothing here:
tests/test_fog_gpu.py does that.  Needs a HIP device."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, FogParams, LIGHT_SKY, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("fog_bench.py needs a HIP device")
    ctx = Context(0)
    W, H = 3840, 2160
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 4, 3, LIGHT_SKY
    app.Draw()
    torch.cuda.synchronize()
    src, nbytes = app.mBackBuffer.clone(), W * H * 4
    dst = torch.zeros_like(src)
    lit = torch.zeros_like(src)
    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.current_stream(ctx.device)
    f = app.frame_desc()
    maps = (C.c_void_p * 4)(*[app.mShadowMap.mShadowMap[i].data_ptr() for i in range(4)])

    def fog(n, density=None):
        p = FogParams.default(steps=n) if density is None else FogParams.default(steps=n, density=density)
        return lambda: app.apply_fog(src, dst, params=p)

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def light():
        check(lib.crychic_deferred_light(ctx.handle, C.byref(app.mMainPassCB), f.g0_dev, f.g1_dev, f.g2_dev, f.depth_dev, f.ambient0_dev, maps,
                                         f.shadowDim, f.cube_dev, f.cubeDim, lit.data_ptr(), None, W, H, 0, H, 3, f.pcfSearchRadius, f.flags,
                                         stream.cuda_stream))

    def draw():
        app.fog = None
        app.Draw()

    def draw_fog():
        app.fog = True
        app.Draw()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    legs = {"fog_n8": fog(8), "fog_n16": fog(16), "fog_n32": fog(32), "fog_n64": fog(64), "memcpy": memcpy, "light": light,
            "fog_density0": fog(16, 0.0), "draw": draw, "draw_fog": draw_fog}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    app.fog = None
    med = statistics.median
    legs["fog_n16"]()                           # dst now holds the pass's frame at the defaults
    torch.cuda.synchronize()
    out = {"metric": "fog", "device": ctx.device_name, "frame": [W, H], "plane_bytes": nbytes, "shadow_dim": 4096, "runs": args.steps}
    for k in ("fog_n8", "fog_n16", "fog_n32", "fog_n64", "memcpy", "light", "fog_density0"):
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    for n in (8, 16, 32, 64):
        out["gather_ns_n%d" % n] = round(1e6 * (med(times["fog_n%d" % n]) - med(times["fog_density0"])) / (W * H * n), 5)
    out["draw_ms"], out["draw_fog_ms"] = round(med(times["draw"]), 4), round(med(times["draw_fog"]), 4)
    out["draw_fog_minus_draw_us"] = round(1e3 * (med(times["draw_fog"]) - med(times["draw"])), 2)
    out["fog_n16_over_light"] = round(med(times["fog_n16"]) / med(times["light"]), 3)
    out["pixels_changed_share"] = round(float((dst != src).any(-1).float().mean().item()), 6)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
