"""Cost of the post-process anti-aliasing pass on the benchmark's 4K frame; prints one JSON line.

    python tools/post_aa_bench.py [--steps 200] [--warmup 10] [--out profiles/post_aa_bench.txt]

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map), lit once;
then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round by round in one process, the
median of --steps rounds each:
  (a) antialias_us    crychic_antialias of that frame alone (33.2 MB read, 33.2 MB written at the least);
  (b) memcpy_us       hipMemcpyAsync, device to device, of the same 33.2 MB plane -- the yardstick for "read once, write once";
  (c) draw_ms / draw_aa_ms   Crychic.Draw() without and with antiAliasing set;
  (d) antialias_no_edges_us  (a) with absMin = 0xFFFFFFFF, so that every pixel is an early copy: the fill, the barrier, the threshold
      tests and the stores without any edge path -- what the streaming skeleton of the kernel costs on its own.
Each of (a) and (b) is also timed as 50 calls back to back between one pair of events (the *_batch_us figures: per call, without the
gap an event pair adds).  The output of (a) is compared with nothing here: tests/test_post_aa_gpu.py does that.  Needs a HIP device."""
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
    from crychic_renderer_amd import AAParams, Context, Crychic, LIGHT_SKY, scene
    if not torch.cuda.is_available():
        sys.exit("post_aa_bench.py needs a HIP device")
    ctx = Context(0)
    W, H = 3840, 2160
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 4, 3, LIGHT_SKY
    app.Draw()
    torch.cuda.synchronize()
    src, nbytes = app.mBackBuffer, W * H * 4
    dst = torch.zeros_like(src)
    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.current_stream(ctx.device)

    def antialias():
        app.antialias(src, dst)

    no_edges = AAParams.default(absMin=0xFFFFFFFF)

    def antialias_no_edges():
        app.antialias(src, dst, params=no_edges)

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def draw():
        app.antiAliasing = None
        app.Draw()

    def draw_aa():
        app.antiAliasing = True
        app.Draw()

    def timed(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n          # ms per call

    legs = {"antialias": antialias, "memcpy": memcpy, "draw": draw, "draw_aa": draw_aa, "antialias_no_edges": antialias_no_edges}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    batch = {k: [] for k in ("antialias", "memcpy", "antialias_no_edges")}
    for _ in range(max(1, args.steps // 20)):
        for k in batch:
            batch[k].append(timed(legs[k], 50))
    app.antiAliasing = None
    med = statistics.median
    antialias()                                 # dst now holds the pass's frame, not the copy
    torch.cuda.synchronize()
    out = {"metric": "post_aa", "device": ctx.device_name, "frame": [W, H], "plane_bytes": nbytes, "runs": args.steps,
           "antialias_us": round(1e3 * med(times["antialias"]), 2), "memcpy_us": round(1e3 * med(times["memcpy"]), 2),
           "antialias_us_min_max": [round(1e3 * min(times["antialias"]), 2), round(1e3 * max(times["antialias"]), 2)],
           "memcpy_us_min_max": [round(1e3 * min(times["memcpy"]), 2), round(1e3 * max(times["memcpy"]), 2)],
           "antialias_batch_us": round(1e3 * med(batch["antialias"]), 2), "memcpy_batch_us": round(1e3 * med(batch["memcpy"]), 2),
           "draw_ms": round(med(times["draw"]), 4), "draw_aa_ms": round(med(times["draw_aa"]), 4)}
    out["antialias_no_edges_us"] = round(1e3 * med(times["antialias_no_edges"]), 2)
    out["antialias_no_edges_batch_us"] = round(1e3 * med(batch["antialias_no_edges"]), 2)
    out["antialias_over_memcpy"] = round(med(times["antialias"]) / med(times["memcpy"]), 3)
    out["antialias_over_memcpy_batch"] = round(med(batch["antialias"]) / med(batch["memcpy"]), 3)
    out["antialias_gb_per_s"] = round(2 * nbytes / (1e-3 * med(batch["antialias"])) / 1e9, 1)      # the streaming floor's bytes over the time
    out["draw_aa_minus_draw_us"] = round(1e3 * (med(times["draw_aa"]) - med(times["draw"])), 2)
    out["pixels_changed_share"] = round(float((dst != src).any(-1).float().mean().item()), 6)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
