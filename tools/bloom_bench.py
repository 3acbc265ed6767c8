"""Cost of the bloom pass on the benchmark's 4K frame; prints one JSON line.

    python tools/bloom_bench.py [--steps 200] [--warmup 10] [--out profiles/bloom_bench.txt]
    python tools/bloom_bench.py --loop 50          # crychic_bloom at the defaults 50 times and nothing timed: the run to put under
                                                   # rocprofv3 --kernel-trace --stats for each kernel's share

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map, four
4096 x 4096 cascades), lit once; then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round
by round in one process, the median of --steps rounds each:
  (a) bloom_us, bloom_l1_us, bloom_l4_us, bloom_l8_us   crychic_bloom of that frame alone at the defaults (6 levels) and at 1, 4, 8;
  (b) pyramid_us, composite_us, composite_inplace_us    the two halves of (a) at the defaults, each alone;
  (c) bloom_dark_us             (a) with threshold 255: every downsample tile takes the zero shortcut and every composite wavefront
                                adds nothing -- the streaming skeleton;
  (d) memcpy_us                 hipMemcpyAsync, device to device, of the same 33.2 MB plane (4 N bytes read, 4 N written);
  (e) light_us                  crychic_deferred_light of the same frame;
  (f) draw_ms / draw_bloom_ms   Crychic.Draw() without and with bloom set (the defaults).
algorithmic_bytes: 17 N for N pixels -- 4 N + 2 N for the first downsample, 4 N + 2 N + 4 N for the composite, about N for the smaller
levels; bandwidth_share: (algorithmic_bytes / bloom_us) / (8 N / memcpy_us), the achieved fraction of the copy leg's bandwidth.
over_threshold_share: the frame's texels with a weight above 0 at the defaults; pixels_changed_share: those the pass changes.  The
output is compared with nothing here: tests/test_bloom_gpu.py does that.  Needs a HIP device."""
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
    ap.add_argument("--loop", type=int, default=0, help="only run crychic_bloom at the defaults this many times (for a kernel trace)")
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import BloomParams, BLOOM_MAX_LEVELS, Context, Crychic, LIGHT_SKY, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("bloom_bench.py needs a HIP device")
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
    inplace = src.clone()
    need = int(lib.crychic_bloom_workspace_bytes(W, H, BLOOM_MAX_LEVELS))
    ws = torch.zeros((need,), dtype=torch.uint8, device=ctx.device)
    stream = torch.cuda.current_stream(ctx.device)

    def bloom(**kw):
        p = BloomParams.default(**kw)
        return lambda: check(lib.crychic_bloom(ctx.handle, src.data_ptr(), dst.data_ptr(), W, H, C.byref(p), ws.data_ptr(), need, stream.cuda_stream))

    if args.loop:
        fn = bloom()
        for _ in range(args.loop):
            fn()
        torch.cuda.synchronize()
        print("ran crychic_bloom %d times" % args.loop)
        ctx.close()
        return

    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    f = app.frame_desc()
    maps = (C.c_void_p * 4)(*[app.mShadowMap.mShadowMap[i].data_ptr() for i in range(4)])
    defaults = BloomParams.default()

    def pyramid():
        check(lib.crychic_bloom_pyramid(ctx.handle, src.data_ptr(), W, H, C.byref(defaults), ws.data_ptr(), need, stream.cuda_stream))

    def composite(out):
        return lambda: check(lib.crychic_bloom_composite(ctx.handle, (inplace if out is inplace else src).data_ptr(), out.data_ptr(), W, H, 0, H,
                                                         C.byref(defaults), ws.data_ptr(), need, stream.cuda_stream))

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def light():
        check(lib.crychic_deferred_light(ctx.handle, C.byref(app.mMainPassCB), f.g0_dev, f.g1_dev, f.g2_dev, f.depth_dev, f.ambient0_dev, maps,
                                         f.shadowDim, f.cube_dev, f.cubeDim, lit.data_ptr(), None, W, H, 0, H, 3, f.pcfSearchRadius, f.flags,
                                         stream.cuda_stream))

    def draw():
        app.bloom = None
        app.Draw()

    def draw_bloom():
        app.bloom = True
        app.Draw()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    # the composite legs come behind a pyramid at the defaults: level 1 of the workspace is what they read
    legs = {"bloom_l1": bloom(levels=1), "bloom_l4": bloom(levels=4), "bloom_l8": bloom(levels=8), "bloom_dark": bloom(threshold=255), "bloom": bloom(),
            "pyramid": pyramid, "composite": composite(dst), "composite_inplace": composite(inplace), "memcpy": memcpy, "light": light, "draw": draw,
            "draw_bloom": draw_bloom}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        inplace.copy_(src)
        for k, fn in legs.items():
            times[k].append(timed(fn))
    app.bloom = None
    med = statistics.median
    legs["bloom"]()                             # dst now holds the pass's frame at the defaults
    torch.cuda.synchronize()
    out = {"metric": "bloom", "device": ctx.device_name, "frame": [W, H], "plane_bytes": nbytes, "workspace_bytes": need, "runs": args.steps}
    for k in ("bloom", "bloom_l1", "bloom_l4", "bloom_l8", "bloom_dark", "pyramid", "composite", "composite_inplace", "memcpy", "light"):
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    out["draw_ms"], out["draw_bloom_ms"] = round(med(times["draw"]), 4), round(med(times["draw_bloom"]), 4)
    out["draw_bloom_minus_draw_us"] = round(1e3 * (med(times["draw_bloom"]) - med(times["draw"])), 2)
    out["bloom_over_light"] = round(med(times["bloom"]) / med(times["light"]), 3)
    out["algorithmic_bytes"] = 17 * W * H
    out["bandwidth_share"] = round((17 * W * H / med(times["bloom"])) / (2 * nbytes / med(times["memcpy"])), 3)
    out["bandwidth_share_dark"] = round((17 * W * H / med(times["bloom_dark"])) / (2 * nbytes / med(times["memcpy"])), 3)
    s = src.to(torch.int32)
    luma = 77 * s[..., 0] + 150 * s[..., 1] + 29 * s[..., 2]
    out["over_threshold_share"] = round(float(((luma - 256 * defaults.threshold) >= defaults.knee).float().mean().item()), 6)
    out["pixels_changed_share"] = round(float((dst != src).any(-1).float().mean().item()), 6)
    out["mean_abs_change"] = round(float((dst.to(torch.int32) - s).abs().float().mean().item()), 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
