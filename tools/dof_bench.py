"""Cost of the depth-of-field pass on the benchmark's 4K frame; prints one JSON line.

    python tools/dof_bench.py [--steps 200] [--warmup 10] [--out profiles/dof_bench.txt]

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (blurCount 4, 3 directional lights, sky, 256-texel cube map, four
4096 x 4096 cascades), lit once; then, timed with HIP events on the context's stream after --warmup untimed rounds, alternated round
by round in one process, the median of --steps rounds each:
  (a) dof_r2_us .. dof_r8_us    crychic_dof of that frame alone at R = 2, 4, 8, the other parameters default (aperture 6);
  (b) dof_wide_r8_us            (a) at R = 8 with aperture 64: nearly every pixel gathers all 197 taps -- the worst case;
  (c) dof_aperture0_us          (a) at R = 8 with aperture 0: every workgroup takes the copy shortcut -- the staging skeleton;
  (d) memcpy_us                 hipMemcpyAsync, device to device, of the same 33.2 MB plane;
  (e) light_us                  crychic_deferred_light of the same frame;
  (f) draw_ms / draw_dof_ms     Crychic.Draw() without and with depthOfField set (the defaults).
tap_ps_*: ((a) or (b) - (c)) / (W H taps of the disc), an upper bound of the cost of one tap of one pixel (the cut at cmax + 8 skips
some).  coc_*: the share of the frame's texels with c = 0, with 0 < c < 16 R and with c = 16 R at the defaults.  The output of (a) is
compared with nothing here: tests/test_dof_gpu.py does that.  Needs a HIP device."""
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
    from crychic_renderer_amd import Context, Crychic, DofParams, LIGHT_SKY, check, lib, scene
    if not torch.cuda.is_available():
        sys.exit("dof_bench.py needs a HIP device")
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

    def dof(radius, aperture=None):
        p = DofParams.default(radius=radius, aperture=aperture)
        return lambda: app.depth_of_field(src, dst, params=p)

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def light():
        check(lib.crychic_deferred_light(ctx.handle, C.byref(app.mMainPassCB), f.g0_dev, f.g1_dev, f.g2_dev, f.depth_dev, f.ambient0_dev, maps,
                                         f.shadowDim, f.cube_dev, f.cubeDim, lit.data_ptr(), None, W, H, 0, H, 3, f.pcfSearchRadius, f.flags,
                                         stream.cuda_stream))

    def draw():
        app.depthOfField = None
        app.Draw()

    def draw_dof():
        app.depthOfField = True
        app.Draw()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    legs = {"dof_r2": dof(2), "dof_r4": dof(4), "dof_r8": dof(8), "dof_wide_r8": dof(8, 64.0), "dof_aperture0": dof(8, 0.0), "memcpy": memcpy,
            "light": light, "draw": draw, "draw_dof": draw_dof}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    app.depthOfField = None
    med = statistics.median
    legs["dof_r8"]()                            # dst now holds the pass's frame at the defaults
    torch.cuda.synchronize()
    out = {"metric": "dof", "device": ctx.device_name, "frame": [W, H], "plane_bytes": nbytes, "runs": args.steps}
    for k in ("dof_r2", "dof_r4", "dof_r8", "dof_wide_r8", "dof_aperture0", "memcpy", "light"):
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    for k, taps in (("dof_r2", 13), ("dof_r4", 49), ("dof_r8", 197), ("dof_wide_r8", 197)):
        out["tap_ps_" + k[4:]] = round(1e9 * (med(times[k]) - med(times["dof_aperture0"])) / (W * H * taps), 3)
    out["draw_ms"], out["draw_dof_ms"] = round(med(times["draw"]), 4), round(med(times["draw_dof"]), 4)
    out["draw_dof_minus_draw_us"] = round(1e3 * (med(times["draw_dof"]) - med(times["draw"])), 2)
    out["dof_r8_over_light"] = round(med(times["dof_r8"]) / med(times["light"]), 3)
    out["pixels_changed_share"] = round(float((dst != src).any(-1).float().mean().item()), 6)
    # the frame's circles of confusion at the defaults, with the definition's arithmetic in torch (float32, one rounding per operation)
    p = DofParams.default()
    A, B = torch.tensor(app.mMainPassCB.Proj[10], dtype=torch.float32), torch.tensor(app.mMainPassCB.Proj[11], dtype=torch.float32)
    v = (app.mDepthStencilBuffer & 0xFFFFFF).to(torch.float64) / 16777215.0
    x = (v.to(torch.float32) - A.to(v.device)) * (torch.tensor(p.focusDistance, dtype=torch.float32) / B).to(v.device)
    c = (torch.clamp((1.0 - x).abs() * (p.aperture * 16.0), 0.0, 16.0 * p.maxRadius) + 0.5).to(torch.int32)
    out["coc_zero_share"] = round(float((c == 0).float().mean().item()), 4)
    out["coc_full_share"] = round(float((c == 16 * p.maxRadius).float().mean().item()), 4)
    out["coc_mean_sixteenths"] = round(float(c.float().mean().item()), 2)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
