"""Cost of the motion blur pass on the benchmark's 4K frame; prints one JSON line.

    python tools/motion_blur_bench.py [--steps 200] [--warmup 10] [--out profiles/motion_blur_bench.txt]
    python tools/motion_blur_bench.py --loop 50        # crychic_motion_blur with a panning camera at N = 8 50 times and nothing timed:
                                                       # the run to put under a profiler

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map, four
4096 x 4096 cascades), lit once; then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round
by round in one process, the median of --steps rounds each:
  (a) pan_n4_us .. pan_n32_us   crychic_motion_blur (both launches) with a previous camera turned by about 12 pixels at the frame's
                                centre, shutter 256, R = 16, at N = 4, 8, 16 and 32: every tile gathers;
  (b) still_us                  the same with identical matrices: every tile is copied with 16-byte loads and stores;
  (c) velocity_us               crychic_motion_blur_velocity alone (panning);
  (d) gather_n8_us              crychic_motion_blur_gather alone over the panning workspace at N = 8;
  (e) memcpy_us                 hipMemcpyAsync, device to device, of the same 33.2 MB RGBA8 plane (4 P bytes read, 4 P written);
  (f) light_us                  crychic_deferred_light of the same frame;
  (g) draw_ms / draw_mb_ms      Crychic.Draw() without and with motionBlur set (the defaults, the panning camera).
compulsory_bytes: 24 P for P pixels -- 4 P depth read and 8 P workspace written by the velocity launch, 8 P workspace and 4 P frame read
once and 4 P frame written by the gather (the samples of neighbouring pixels overlap: what they cost beyond that is cache traffic);
gathers: P N loads of 8 bytes and P N of 4.  The output is compared with nothing here: tests/test_motion_blur_gpu.py does that.  Needs
a HIP device."""
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
    ap.add_argument("--loop", type=int, default=0, help="only run crychic_motion_blur with a panning camera this many times")
    args = ap.parse_args()
    import math
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, MotionBlurParams, PassConstants, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("motion_blur_bench.py needs a HIP device")
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
    need = int(lib.crychic_motion_blur_workspace_bytes(W, H))
    ws = torch.zeros((need,), dtype=torch.uint8, device=ctx.device)
    stream = torch.cuda.current_stream(ctx.device)
    cur = (C.c_float * 16)(*app.mMainPassCB.ViewProj)
    cam = scene.default_camera(W, H)
    a = 12.0 * 2.0 * math.tan(0.125 * math.pi) / H          # about 12 pixels at the frame's centre (fovY = pi / 4)
    cam.look[:] = (math.sin(a), 0.0, math.cos(a))
    moved = PassConstants()
    st = (C.c_float * 64)()
    dirs = (C.c_float * 9)(*[v for d in scene.BASE_LIGHT_DIRS for v in d])
    check(lib.crychic_update_main_pass_cb(C.byref(cam), W, H, st, dirs, C.byref(moved)))
    prev = (C.c_float * 16)(*moved.ViewProj)
    depth = app.mDepthStencilBuffer.data_ptr()

    def blur(prev_m, n):
        p = MotionBlurParams.default(shutter=256, samples=n, maxRadius=16)
        return lambda: check(lib.crychic_motion_blur(ctx.handle, C.byref(app.mMainPassCB), cur, prev_m, depth, src.data_ptr(), dst.data_ptr(), W, H,
                                                     C.byref(p), ws.data_ptr(), need, stream.cuda_stream))

    p8 = MotionBlurParams.default(shutter=256, samples=8, maxRadius=16)

    def velocity():
        check(lib.crychic_motion_blur_velocity(ctx.handle, C.byref(app.mMainPassCB), cur, prev, depth, W, H, C.byref(p8), ws.data_ptr(), need,
                                               stream.cuda_stream))

    def gather():
        check(lib.crychic_motion_blur_gather(ctx.handle, src.data_ptr(), dst.data_ptr(), W, H, 0, H, C.byref(p8), ws.data_ptr(), need, stream.cuda_stream))

    if args.loop:
        fn = blur(prev, 8)
        for _ in range(args.loop):
            fn()
        torch.cuda.synchronize()
        print("ran crychic_motion_blur %d times" % args.loop)
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
        app.motionBlur = None
        app.Draw()

    def draw_mb():
        app.motionBlur = True
        app.Draw()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    app.set_frame_view_proj(tuple(prev))
    app.set_frame_view_proj(tuple(cur))
    # the velocity leg stands in front of the gather leg, so that the gather leg reads the panning workspace
    legs = {"pan_n4": blur(prev, 4), "pan_n8": blur(prev, 8), "pan_n16": blur(prev, 16), "pan_n32": blur(prev, 32), "still": blur(cur, 8),
            "velocity": velocity, "gather_n8": gather, "memcpy": memcpy, "light": light}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
        draw()
        draw_mb()
    torch.cuda.synchronize()
    moving = float((ws[:W * H * 8].view(torch.int32)[::2] != 0).float().mean())         # after the gather leg: the panning workspace
    times = {k: [] for k in legs}
    times["draw"], times["draw_mb"] = [], []
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
        times["draw"].append(timed(draw))
        times["draw_mb"].append(timed(draw_mb))
    app.motionBlur = None
    med = statistics.median
    out = {"metric": "motion_blur", "device": ctx.device_name, "frame": [W, H], "plane_bytes": nbytes, "workspace_bytes": need, "runs": args.steps,
           "moving_pixels_share": round(moving, 4)}
    for k in legs:
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    out["draw_ms"], out["draw_mb_ms"] = round(med(times["draw"]), 4), round(med(times["draw_mb"]), 4)
    out["draw_mb_minus_draw_us"] = round(1e3 * (med(times["draw_mb"]) - med(times["draw"])), 2)
    out["pan_n8_over_light"] = round(med(times["pan_n8"]) / med(times["light"]), 3)
    out["compulsory_bytes"] = 24 * W * H
    copy_bw = 2 * nbytes / med(times["memcpy"])
    for k in ("pan_n4", "pan_n8", "pan_n16", "pan_n32", "still"):
        out["compulsory_bandwidth_share_" + k] = round((24 * W * H / med(times[k])) / copy_bw, 3)
    out["us_per_sample_pair_n8_to_n32"] = round(1e3 * (med(times["pan_n32"]) - med(times["pan_n8"])) / 24, 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
