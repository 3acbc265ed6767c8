"""Cost of the glossy screen-space reflections on the benchmark's 4K frame; prints one JSON line.

    python tools/ssr_gloss_bench.py [--steps 100] [--warmup 10] [--camera reference|covered] [--out profiles/ssr_gloss_bench.txt]

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (tools/ssr_bench.py's set-up; --camera covered: its covered camera),
lit once; then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round by round in one
process, the median of --steps rounds each, with min .. max:
  (a) pyramid_l3_us, _l6_us, _l8_us   crychic_ssr_pyramid of that frame alone at 3, 6 and 8 levels (2, 5 and 7 launches);
  (b) ssr_n*_us / glossy_n*_us        crychic_ssr against crychic_ssr_glossy (coneScale --cone, 6 levels, the pyramid built before the
                                      clock starts) at N = 16, 32, 64 steps, the other parameters default;
  (c) glossy_cone0_n32_us             (b) at coneScale 0: no wavefront fetches from the pyramid;
  (d) memcpy_us                       hipMemcpyAsync, device to device, of the same 33.2 MB plane;
  (e) draw_ssr_ms / draw_gloss_ms     Crychic.Draw() with ssr against ssr + ssrGloss (coneScale --cone, 6 levels).
The outputs are compared with nothing here: tests/test_ssr_gloss_gpu.py does that.  Needs a HIP device."""
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cone", type=float, default=0.7)
    ap.add_argument("--camera", choices=["reference", "covered"], default="reference")
    ap.add_argument("--out", default="", help="also append the JSON to this file")
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, SsrGlossParams, SsrParams, LIGHT_SKY, scene
    if not torch.cuda.is_available():
        sys.exit("ssr_gloss_bench.py needs a HIP device")
    ctx = Context(0)
    W, H = 3840, 2160
    consts = scene.Constants(W, H, 4096, cam=scene.covered_camera(W, H)) if args.camera == "covered" else None
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device), consts=consts)
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 4, 3, LIGHT_SKY
    app.Draw()
    torch.cuda.synchronize()
    src, nbytes = app.mBackBuffer.clone(), W * H * 4
    dst = torch.zeros_like(src)
    sharp = torch.zeros_like(src)
    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.current_stream(ctx.device)
    gloss = SsrGlossParams.default(coneScale=args.cone, levels=6)
    app.ssr_pyramid(src, levels=6)              # what the glossy legs read

    def pyramid(levels):
        return lambda: app.ssr_pyramid(src, levels=levels)

    def ssr(n):
        p = SsrParams.default(steps=n)
        return lambda: app.screen_space_reflections(src, sharp, params=p)

    def glossy(n, g=gloss):
        p = SsrParams.default(steps=n)
        return lambda: app.screen_space_reflections(src, dst, params=p, gloss=g)

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def draw_ssr():
        app.ssr, app.ssrGloss = True, None
        app.Draw()

    def draw_gloss():
        app.ssr, app.ssrGloss = True, gloss
        app.Draw()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    # the pyramid legs come last in a round and the 6-level one last of them, so the glossy legs of the next round read 6 levels
    legs = {"ssr_n16": ssr(16), "glossy_n16": glossy(16), "ssr_n32": ssr(32), "glossy_n32": glossy(32), "ssr_n64": ssr(64), "glossy_n64": glossy(64),
            "glossy_cone0_n32": glossy(32, SsrGlossParams.default(coneScale=0.0, levels=6)), "memcpy": memcpy, "draw_ssr": draw_ssr, "draw_gloss": draw_gloss,
            "pyramid_l3": pyramid(3), "pyramid_l8": pyramid(8), "pyramid_l6": pyramid(6)}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    app.ssr, app.ssrGloss = None, None
    med = statistics.median
    legs["ssr_n32"]()
    legs["glossy_n32"]()                        # sharp and dst now hold the two passes' frames at N = 32
    torch.cuda.synchronize()
    out = {"metric": "ssr_gloss", "device": ctx.device_name, "frame": [W, H], "camera": args.camera, "coneScale": args.cone, "levels": 6,
           "plane_bytes": nbytes, "pyramid_bytes_l6": int(app.mSsrPyramid.numel()), "runs": args.steps}
    for k in legs:
        if k.startswith("draw"):
            continue
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    for n in (16, 32, 64):
        out["glossy_minus_ssr_n%d_us" % n] = round(1e3 * (med(times["glossy_n%d" % n]) - med(times["ssr_n%d" % n])), 2)
    out["pyramid_l6_over_memcpy"] = round(med(times["pyramid_l6"]) / med(times["memcpy"]), 3)
    out["draw_ssr_ms"], out["draw_gloss_ms"] = round(med(times["draw_ssr"]), 4), round(med(times["draw_gloss"]), 4)
    out["draw_ms_min_max"] = {k: [round(min(times[k]), 4), round(max(times[k]), 4)] for k in ("draw_ssr", "draw_gloss")}
    out["draw_gloss_minus_draw_ssr_us"] = round(1e3 * (med(times["draw_gloss"]) - med(times["draw_ssr"])), 2)
    out["pixels_changed_by_the_cone_share"] = round(float((dst != sharp).any(-1).float().mean().item()), 6)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
