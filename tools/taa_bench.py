"""Cost of the temporal anti-aliasing pass on the benchmark's 4K frame; prints one JSON line.

    python tools/taa_bench.py [--steps 200] [--warmup 10] [--out profiles/taa_bench.txt]
    python tools/taa_bench.py --loop 50            # crychic_taa with a still camera 50 times and nothing timed: the run to put under a
                                                   # profiler

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map, four
4096 x 4096 cascades), lit once; then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round
by round in one process, the median of --steps rounds each:
  (a) taa_still_us      crychic_taa of that frame with identical matrices: every wavefront drops the three weightless taps;
  (b) taa_pan_us        the same with a previous camera turned by a fraction of a pixel: four taps per pixel;
  (c) taa_reset_us      the same with CRYCHIC_TAA_RESET: the history is not read -- the streaming skeleton;
  (d) memcpy_us         hipMemcpyAsync, device to device, of the same 33.2 MB RGBA8 plane (4 N bytes read, 4 N written);
  (e) light_us          crychic_deferred_light of the same frame;
  (f) draw_ms / draw_taa_ms   Crychic.Draw() without and with temporalAA set (the defaults, a still camera).
algorithmic_bytes: 28 N for N pixels -- 4 N frame, 4 N depth and 8 N history read, 8 N history and 4 N frame written (20 N with
RESET); bandwidth_share: (algorithmic_bytes / time) / (8 N / memcpy_us), the achieved fraction of the copy leg's bandwidth.  The
output is compared with nothing here: tests/test_taa_gpu.py does that.  Needs a HIP device."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    ap.add_argument("--loop", type=int, default=0, help="only run crychic_taa with a still camera this many times")
    args = ap.parse_args()
    import math
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, TaaParams, TAA_RESET, PassConstants, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("taa_bench.py needs a HIP device")
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
    hin = (src.to(torch.int32) * 256).to(torch.int16)       # the history a still camera converges to: 8.8 fixed point of the frame
    hout = torch.zeros_like(hin)
    stream = torch.cuda.current_stream(ctx.device)
    cur = (C.c_float * 16)(*app.mMainPassCB.ViewProj)
    cam = scene.default_camera(W, H)
    a = 0.37 / W
    cam.look[:] = (math.sin(a), 0.0, math.cos(a))
    moved = PassConstants()
    st = (C.c_float * 64)()
    dirs = (C.c_float * 9)(*[v for d in scene.BASE_LIGHT_DIRS for v in d])
    check(lib.crychic_update_main_pass_cb(C.byref(cam), W, H, st, dirs, C.byref(moved)))
    prev = (C.c_float * 16)(*moved.ViewProj)

    def taa(prev_m, flags=0):
        p = TaaParams.default(flags=flags)
        return lambda: check(lib.crychic_taa(ctx.handle, C.byref(app.mMainPassCB), cur, prev_m, app.mDepthStencilBuffer.data_ptr(), src.data_ptr(),
                                             hin.data_ptr(), hout.data_ptr(), dst.data_ptr(), W, H, 0, H, C.byref(p), stream.cuda_stream))

    if args.loop:
        fn = taa(cur)
        for _ in range(args.loop):
            fn()
        torch.cuda.synchronize()
        print("ran crychic_taa %d times" % args.loop)
        ctx.close()
        return

    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    f = app.frame_desc()
    maps = (C.c_void_p * 4)(*[app.mShadowMap.mShadowMap[i].data_ptr() for i in range(4)])

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def light():
        check(lib.crychic_deferred_light(ctx.handle, C.byref(app.mMainPassCB), f.g0_dev, f.g1_dev, f.g2_dev, f.depth_dev, f.ambient0_dev, maps,
                                         f.shadowDim, f.cube_dev, f.cubeDim, lit.data_ptr(), None, W, H, 0, H, 3, f.pcfSearchRadius, f.flags,
                                         stream.cuda_stream))

    def draw():
        app.temporalAA = None
        app.Draw()

    def draw_taa():
        if not app.temporalAA:
            app.temporalAA = True
            app.Draw()                          # the RESET frame of the switch going on: not the steady state
        app.Draw()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    legs = {"taa_still": taa(cur), "taa_pan": taa(prev), "taa_reset": taa(cur, TAA_RESET), "memcpy": memcpy, "light": light}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
        draw()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    times["draw"], times["draw_taa"] = [], []
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    # Draw() off and on in blocks, so that the switch's RESET frame stays out of the timed calls
    for _ in range(4):
        draw()
        for _ in range(args.steps // 4):
            times["draw"].append(timed(draw))
        draw_taa()
        for _ in range(args.steps // 4):
            times["draw_taa"].append(timed(draw_taa))
    app.temporalAA = None
    med = statistics.median
    out = {"metric": "taa", "device": ctx.device_name, "frame": [W, H], "plane_bytes": nbytes, "history_bytes": 2 * nbytes, "runs": args.steps}
    for k in legs:
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    out["draw_ms"], out["draw_taa_ms"] = round(med(times["draw"]), 4), round(med(times["draw_taa"]), 4)
    out["draw_taa_minus_draw_us"] = round(1e3 * (med(times["draw_taa"]) - med(times["draw"])), 2)
    out["taa_still_over_light"] = round(med(times["taa_still"]) / med(times["light"]), 3)
    out["algorithmic_bytes"] = 28 * W * H
    copy_bw = 2 * nbytes / med(times["memcpy"])
    for k, n in (("taa_still", 28), ("taa_pan", 28), ("taa_reset", 20)):
        out["bandwidth_share_" + k[4:]] = round((n * W * H / med(times[k])) / copy_bw, 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
