"""Cost of the colour grade on the benchmark's 4K frame; prints one JSON line.

    python tools/grade_bench.py [--steps 200] [--warmup 10] [--out profiles/grade_bench.txt]

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map), lit once;
then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round by round in one process, the
median of --steps rounds each:
  (a) grade17_us, grade33_us   crychic_grade of that frame alone through the table of one non-trivial look at N = 17 and at N = 33
      (33.2 MB read, 33.2 MB written, and one fill of the table per workgroup);
  (b) memcpy_us       hipMemcpyAsync, device to device, of the same 33.2 MB plane -- the yardstick for "read once, write once";
  (c) draw_ms / draw_grade_ms   Crychic.Draw() with colourGrade unset and set (N = 33).
Each of (a) and (b) is also timed as 50 calls back to back between one pair of events (the *_batch_us figures: per call, without the
gap an event pair adds).  The output of (a) is compared with nothing here: tests/test_grade_gpu.py does that.  Needs a HIP device."""
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
    from crychic_renderer_amd import Context, Crychic, GradeParams, LIGHT_SKY, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("grade_bench.py needs a HIP device")
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
    look = GradeParams.default(slope=(1.2, 1.0, 0.8), offset=(0.03, 0.0, -0.02), power=(0.9, 1.0, 1.2), saturation=1.3)
    tables = {}
    for N in (17, 33):
        buf = (C.c_uint8 * (4 * N ** 3))()
        check(lib.crychic_grade_build_lut(C.byref(look), N, buf, len(buf)))
        tables[N] = torch.frombuffer(buf, dtype=torch.uint8).reshape(N, N, N, 4).to(ctx.device)
    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.current_stream(ctx.device)

    def grade(N):
        def go():
            check(lib.crychic_grade(ctx.handle, src.data_ptr(), dst.data_ptr(), W, H, 0, H, tables[N].data_ptr(), N, stream.cuda_stream))
        return go

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def draw():
        if app.colourGrade is not None:
            app.colourGrade = None
        app.Draw()

    def draw_grade():
        if app.colourGrade is None:
            app.colourGrade = tables[33]
        app.Draw()

    def timed(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n          # ms per call

    legs = {"grade17": grade(17), "grade33": grade(33), "memcpy": memcpy}
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
    # Draw() in two blocks rather than alternated: setting the switch uploads a table, which is no part of a frame
    draws = {}
    for k, fn in (("draw", draw), ("draw_grade", draw_grade)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        draws[k] = [timed(fn) for _ in range(args.steps)]
    app.colourGrade = None
    med = statistics.median
    grade(33)()                                 # dst now holds the pass's frame, not the copy
    torch.cuda.synchronize()
    out = {"metric": "grade", "device": ctx.device_name, "frame": [W, H], "plane_bytes": nbytes, "runs": args.steps}
    for k in legs:
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
        out[k + "_batch_us"] = round(1e3 * med(batch[k]), 2)
    for N in (17, 33):
        out["grade%d_over_memcpy" % N] = round(med(times["grade%d" % N]) / med(times["memcpy"]), 3)
        out["grade%d_over_memcpy_batch" % N] = round(med(batch["grade%d" % N]) / med(batch["memcpy"]), 3)
        out["grade%d_gb_per_s" % N] = round(2 * nbytes / (1e-3 * med(batch["grade%d" % N])) / 1e9, 1)      # the frame's bytes over the time
    out["draw_ms"] = round(med(draws["draw"]), 4)
    out["draw_grade_ms"] = round(med(draws["draw_grade"]), 4)
    out["draw_grade_minus_draw_us"] = round(1e3 * (med(draws["draw_grade"]) - med(draws["draw"])), 2)
    out["pixels_changed_share"] = round(float((dst != src).any(-1).float().mean().item()), 6)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
