"""Cost of the sharpening pass on the benchmark's 4K frame; prints one JSON line.

    python tools/sharpen_bench.py [--steps 200] [--warmup 10] [--out profiles/sharpen_bench.txt]

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map), lit once;
then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round by round in one process, the
median of --steps rounds each:
  (a) sharpen_us, sharpen_narrow_us   crychic_sharpen of that frame alone at strength 256, through the wide kernel and -- the output
      plane 4 bytes past a 16-byte boundary -- through the narrow one (33.2 MB read, 33.2 MB written);
  (b) memcpy_us       hipMemcpyAsync, device to device, of the same 33.2 MB plane -- the yardstick for "read once, write once";
  (c) draw_ms / draw_sharpen_ms   Crychic.Draw() with sharpening unset and set.
Each of (a) and (b) is also timed as 50 calls back to back between one pair of events (the *_batch_us figures: per call, without the
gap an event pair adds).  The output of (a) is compared with nothing here: tests/test_sharpen_gpu.py does that.  Needs a HIP device."""
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
    from crychic_renderer_amd import Context, Crychic, SharpenParams, LIGHT_SKY, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("sharpen_bench.py needs a HIP device")
    ctx = Context(0)
    W, H = 3840, 2160
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 4, 3, LIGHT_SKY
    app.Draw()
    torch.cuda.synchronize()
    src, nbytes = app.mBackBuffer, W * H * 4
    raw = torch.zeros((nbytes + 32,), dtype=torch.uint8, device=src.device)
    base = (-raw.data_ptr()) % 16
    dst, dst_off = raw[base:base + nbytes], raw[base + 4:base + 4 + nbytes]
    strong = SharpenParams.default(strength=256)
    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.current_stream(ctx.device)

    def sharpen(out):
        def go():
            check(lib.crychic_sharpen(ctx.handle, src.data_ptr(), out.data_ptr(), W, H, 0, H, C.byref(strong), stream.cuda_stream))
        return go

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def draw():
        app.sharpening = None
        app.Draw()

    def draw_sharpen():
        app.sharpening = strong
        app.Draw()

    def timed(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n          # ms per call

    legs = {"sharpen": sharpen(dst), "sharpen_narrow": sharpen(dst_off), "memcpy": memcpy}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    batch = {k: [] for k in legs}
    for _ in range(max(1, args.steps // 20)):
        for k in batch:
            batch[k].append(timed(legs[k], 50))
    draws = {"draw": [], "draw_sharpen": []}
    for _ in range(args.warmup):
        draw()
        draw_sharpen()
    torch.cuda.synchronize()
    for _ in range(args.steps):
        draws["draw"].append(timed(draw))
        draws["draw_sharpen"].append(timed(draw_sharpen))
    app.sharpening = None
    med = statistics.median
    sharpen(dst)()                              # dst now holds the pass's frame, not the copy
    torch.cuda.synchronize()
    out = {"metric": "sharpen", "device": ctx.device_name, "frame": [W, H], "plane_bytes": nbytes, "runs": args.steps, "strength": 256, "limit": strong.limit}
    for k in legs:
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
        out[k + "_batch_us"] = round(1e3 * med(batch[k]), 2)
    for k in ("sharpen", "sharpen_narrow"):
        out[k + "_over_memcpy"] = round(med(times[k]) / med(times["memcpy"]), 3)
        out[k + "_over_memcpy_batch"] = round(med(batch[k]) / med(batch["memcpy"]), 3)
    out["sharpen_gb_per_s"] = round(2 * nbytes / (1e-3 * med(batch["sharpen"])) / 1e9, 1)      # the frame's bytes over the time
    out["draw_ms"] = round(med(draws["draw"]), 4)
    out["draw_sharpen_ms"] = round(med(draws["draw_sharpen"]), 4)
    out["draw_sharpen_minus_draw_us"] = round(1e3 * (med(draws["draw_sharpen"]) - med(draws["draw"])), 2)
    out["pixels_changed_share"] = round(float((dst.view(H, W, 4) != src).any(-1).float().mean().item()), 6)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
