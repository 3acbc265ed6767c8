"""Cost of the temporal upsampling from 2560 x 1440 to 3840 x 2160; prints one JSON line.

    python tools/taa_upscale_bench.py [--steps 200] [--warmup 10] [--out FILE]

Two objects over scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map, four 4096 x 4096
cascades), one at 2560 x 1440 and one at 3840 x 2160, each lit once; then, timed with HIP events on the context's stream after
--warmup untimed rounds, alternated round by round in one process, the median of --steps rounds each:
  (a) upscale_still_us   crychic_taa_upscale of the 1440p frame into 4K with identical matrices and the sequence's second jitter;
  (b) upscale_pan_us     the same with a previous camera turned by a fraction of a pixel: four history taps per pixel;
  (c) upscale_reset_us   the same with RESET: the history is not read;
  (d) taa_4k_us          crychic_taa of the 4K frame with identical matrices: the pass this one stands in for;
  (e) memcpy_us          hipMemcpyAsync, device to device, of the 33.2 MB RGBA8 plane of the 4K frame;
  (f) draw_1440p_upscale_ms / draw_4k_taa_ms   Crychic.Draw() at 1440p with temporalUpscale to 4K, bloom and antiAliasing set, and
      Crychic.Draw() at 4K with temporalAA, bloom and antiAliasing set (the defaults, a still camera, steady state).
algorithmic_bytes: 8 Ni for the Ni input pixels (frame and depth) and 20 No for the No output pixels (8 No history read, 8 No history
and 4 No frame written; 12 No with RESET); bandwidth_share: (algorithmic_bytes / time) / (8 No / memcpy_us).  The output is compared
with nothing here: tests/test_taa_upscale_gpu.py does that.  Needs a HIP device."""
import argparse
import ctypes as C
import json
import math
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
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, TaaParams, TaaUpscaleParams, TAA_RESET, PassConstants, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("taa_upscale_bench.py needs a HIP device")
    ctx = Context(0)
    Wi, Hi, Wo, Ho = 2560, 1440, 3840, 2160

    def make(W, H):
        planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
        app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
        app.load_scene(planes)
        app.blurCount, app.numDirLights, app.flags = 4, 3, LIGHT_SKY
        app.Draw()
        return app
    lo, hi = make(Wi, Hi), make(Wo, Ho)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(ctx.device)
    jx, jy = C.c_float(), C.c_float()
    check(lib.crychic_taa_jitter(1, C.byref(jx), C.byref(jy)))

    def matrices(app, W, H):
        cur = (C.c_float * 16)(*app.mMainPassCB.ViewProj)
        cam = scene.default_camera(W, H)
        a = 0.37 / W
        cam.look[:] = (math.sin(a), 0.0, math.cos(a))
        moved = PassConstants()
        st = (C.c_float * 64)()
        dirs = (C.c_float * 9)(*[v for d in scene.BASE_LIGHT_DIRS for v in d])
        check(lib.crychic_update_main_pass_cb(C.byref(cam), W, H, st, dirs, C.byref(moved)))
        return cur, (C.c_float * 16)(*moved.ViewProj)
    cur_lo, prev_lo = matrices(lo, Wi, Hi)
    cur_hi, _ = matrices(hi, Wo, Ho)
    src_lo, src_hi, nbytes = lo.mBackBuffer.clone(), hi.mBackBuffer.clone(), Wo * Ho * 4
    dst = torch.zeros_like(src_hi)
    hin = (src_hi.to(torch.int32) * 256).to(torch.int16)    # a history close to what a still camera converges to
    hout = torch.zeros_like(hin)

    def upscale(prev_m, flags=0):
        p = TaaUpscaleParams.default(flags=flags)
        return lambda: check(lib.crychic_taa_upscale(ctx.handle, C.byref(lo.mMainPassCB), cur_lo, prev_m, jx.value, jy.value, lo.mDepthStencilBuffer.data_ptr(),
                                                     src_lo.data_ptr(), Wi, Hi, hin.data_ptr(), hout.data_ptr(), dst.data_ptr(), Wo, Ho, 0, Ho, C.byref(p),
                                                     stream.cuda_stream))

    def taa_4k():
        p = TaaParams.default()
        return lambda: check(lib.crychic_taa(ctx.handle, C.byref(hi.mMainPassCB), cur_hi, cur_hi, hi.mDepthStencilBuffer.data_ptr(), src_hi.data_ptr(),
                                             hin.data_ptr(), hout.data_ptr(), dst.data_ptr(), Wo, Ho, 0, Ho, C.byref(p), stream.cuda_stream))

    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src_hi.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:   # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    legs = {"upscale_still": upscale(cur_lo), "upscale_pan": upscale(prev_lo), "upscale_reset": upscale(cur_lo, TAA_RESET), "taa_4k": taa_4k(),
            "memcpy": memcpy}
    lo.temporalUpscale, lo.bloom, lo.antiAliasing = (Wo, Ho), True, True
    hi.temporalAA, hi.bloom, hi.antiAliasing = True, True, True
    draws = {"draw_1440p_upscale": lo.Draw, "draw_4k_taa": hi.Draw}
    for _ in range(max(args.warmup, 2)):        # the RESET frames of the switches going on stay out of the timed calls
        for fn in list(legs.values()) + list(draws.values()):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in list(legs) + list(draws)}
    for _ in range(args.steps):
        for k, fn in list(legs.items()) + list(draws.items()):
            times[k].append(timed(fn))
    med = statistics.median
    out = {"metric": "taa_upscale", "device": ctx.device_name, "input": [Wi, Hi], "output": [Wo, Ho], "plane_bytes": nbytes, "runs": args.steps}
    for k in legs:
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    for k in draws:
        out[k + "_ms"] = round(med(times[k]), 4)
        out[k + "_ms_min_max"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
    out["draw_4k_over_1440p"] = round(med(times["draw_4k_taa"]) / med(times["draw_1440p_upscale"]), 3)
    out["upscale_still_over_taa_4k"] = round(med(times["upscale_still"]) / med(times["taa_4k"]), 3)
    out["algorithmic_bytes"] = 8 * Wi * Hi + 20 * Wo * Ho
    copy_bw = 2 * nbytes / med(times["memcpy"])
    for k, n in (("upscale_still", 20), ("upscale_pan", 20), ("upscale_reset", 12)):
        out["bandwidth_share_" + k[8:]] = round(((8 * Wi * Hi + n * Wo * Ho) / med(times[k])) / copy_bw, 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
