"""Cost of the screen-space reflection pass on the benchmark's 4K frame; prints one JSON line.

    python tools/ssr_bench.py [--steps 100] [--warmup 10] [--camera reference|covered] [--out profiles/ssr_bench.txt]

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map, four
4096 x 4096 cascades; --camera covered: bench.py's camera pitched down until every pixel is covered, so that no wavefront leaves at
the sky exit and the rays run along the floor), lit once; then, timed with HIP events on the context's stream after --warmup untimed
rounds, alternated round by round in one process, the median of --steps rounds each:
  (a) ssr_n16_us .. ssr_n64_us  crychic_ssr of that frame alone at N = 16, 32, 64 steps, the other parameters default;
  (b) ssr_rough0_us             (a) at N = 32 with maxRoughness 0: every wavefront takes the copy exit -- the streaming skeleton;
  (c) memcpy_us                 hipMemcpyAsync, device to device, of the same 33.2 MB plane;
  (d) light_us                  crychic_deferred_light of the same frame;
  (e) fog_n16_us                crychic_fog at its defaults (N = 16), out of place -- the nearest existing gather-march;
  (f) draw_ms / draw_ssr_ms     Crychic.Draw() without and with ssr set (the defaults, N = 32).
march_ns_n*: ((a) - (b)) / (W H N), the cost of one step of one pixel had every pixel marched every step (an upper bound on the
share: rays end early).  The output of (a) is compared with nothing here: tests/test_ssr_gpu.py does that.  Needs a HIP device."""
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
    ap.add_argument("--camera", choices=["reference", "covered"], default="reference")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, FogParams, SsrParams, LIGHT_SKY, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("ssr_bench.py needs a HIP device")
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
    lit = torch.zeros_like(src)
    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.current_stream(ctx.device)
    f = app.frame_desc()
    maps = (C.c_void_p * 4)(*[app.mShadowMap.mShadowMap[i].data_ptr() for i in range(4)])

    def ssr(n, **kw):
        p = SsrParams.default(steps=n, **kw)
        return lambda: app.screen_space_reflections(src, dst, params=p)

    def fog():
        app.apply_fog(src, dst, params=FogParams.default())

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def light():
        check(lib.crychic_deferred_light(ctx.handle, C.byref(app.mMainPassCB), f.g0_dev, f.g1_dev, f.g2_dev, f.depth_dev, f.ambient0_dev, maps,
                                         f.shadowDim, f.cube_dev, f.cubeDim, lit.data_ptr(), None, W, H, 0, H, 3, f.pcfSearchRadius, f.flags,
                                         stream.cuda_stream))

    def draw():
        app.ssr = None
        app.Draw()

    def draw_ssr():
        app.ssr = True
        app.Draw()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    legs = {"ssr_n16": ssr(16), "ssr_n32": ssr(32), "ssr_n64": ssr(64), "ssr_rough0": ssr(32, maxRoughness=0.0), "memcpy": memcpy, "light": light,
            "fog_n16": fog, "draw": draw, "draw_ssr": draw_ssr}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    app.ssr = None
    med = statistics.median
    legs["ssr_n32"]()                           # dst now holds the pass's frame at the defaults
    torch.cuda.synchronize()
    out = {"metric": "ssr", "device": ctx.device_name, "frame": [W, H], "camera": args.camera, "plane_bytes": nbytes, "runs": args.steps}
    for k in ("ssr_n16", "ssr_n32", "ssr_n64", "ssr_rough0", "memcpy", "light", "fog_n16"):
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    for n in (16, 32, 64):
        out["march_ns_n%d" % n] = round(1e6 * (med(times["ssr_n%d" % n]) - med(times["ssr_rough0"])) / (W * H * n), 5)
        out["ssr_n%d_over_memcpy" % n] = round(med(times["ssr_n%d" % n]) / med(times["memcpy"]), 3)
        out["ssr_n%d_over_light" % n] = round(med(times["ssr_n%d" % n]) / med(times["light"]), 3)
    out["ssr_rough0_over_memcpy"] = round(med(times["ssr_rough0"]) / med(times["memcpy"]), 3)
    out["ssr_n32_over_fog_n16"] = round(med(times["ssr_n32"]) / med(times["fog_n16"]), 3)
    out["draw_ms"], out["draw_ssr_ms"] = round(med(times["draw"]), 4), round(med(times["draw_ssr"]), 4)
    out["draw_ssr_minus_draw_us"] = round(1e3 * (med(times["draw_ssr"]) - med(times["draw"])), 2)
    out["pixels_changed_share"] = round(float((dst != src).any(-1).float().mean().item()), 6)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
