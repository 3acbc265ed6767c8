"""Cost of the decal pass on the benchmark's 4K frame; prints one JSON line.

    python tools/decal_bench.py [--steps 100] [--warmup 5] [--out profiles/decal_bench.txt]

The 3840 x 2160 frame of scene.make_scene as bench.py draws it (float4 planes), lit once; then, timed with HIP events on the context's
stream after --warmup untimed rounds, alternated round by round in one process, the median (and min .. max) of --steps rounds each:
  skeleton_us            crychic_apply_decals with 64 decals none of which touches the frame (boxes in the air): every wavefront reads
                         its depth words and G0 texels, votes an empty mask and ends -- the pass's streaming skeleton;
  floor1_us .. floor64_us   1, 16 and 64 decals on the floor, every flag set, a 64 x 64 disc with a dent normal map;
  stacked16_us           16 decals on one spot;
  memcpy_us              hipMemcpyAsync, device to device, of the G0 plane (132.7 MB);
  light_us               crychic_deferred_light of the same frame.
The planes are restored to the frame's own in front of every leg, outside the timed region: every decal leg starts from the same
G-buffer, and the light and copy legs see it without decals.  coverage_*: the share of the frame's pixels inside at least one decal of the
leg.  The planes are compared with nothing here: tests/test_decal_gpu.py does that.  Needs a HIP device."""
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    args = ap.parse_args()
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, check, geometry, lib, scene
    if not torch.cuda.is_available():
        sys.exit("decal_bench.py needs a HIP device")
    ctx = Context(0)
    W, H = 3840, 2160
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 4, 3, LIGHT_SKY
    app.Draw()
    torch.cuda.synchronize()
    g0 = app.mDeferred.mGBuffer[0]
    pristine = [g.clone() for g in app.mDeferred.mGBuffer]
    nbytes = g0.numel() * 4
    dst, lit = torch.zeros_like(g0), torch.zeros_like(app.mBackBuffer)
    hip = C.CDLL(None)                          # the HIP runtime the package loaded (torch's), by its global symbols
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.current_stream(ctx.device)
    f = app.frame_desc()
    maps = (C.c_void_p * 4)(*[app.mShadowMap.mShadowMap[i].data_ptr() for i in range(4)])
    textures = [geometry.decal_texture("disc", 64), geometry.decal_texture("dent", 64)]

    def box(x, y, z, half=1.0):
        return geometry.decal_from_box(geometry.decal_box_world((x, y, z), (half, 0.25, half)), (64, 64), 0.5, 0.0, texture=0, normalTexture=1,
                                       flags=15, roughness=0.1, metalness=0.5, opacity=0.8)
    spots = [(-7.0 + 2.0 * (k % 8), 0.0, -9.0 + 3.0 * (k // 8)) for k in range(64)]       # an 8 x 8 grid over the floor in view
    sets = {"skeleton": [box(x, 50.0, z) for x, _, z in spots], "floor1": [box(*spots[9])], "floor16": [box(*p) for p in spots[:16]],
            "floor64": [box(*p) for p in spots], "stacked16": [box(*spots[9]) for _ in range(16)]}
    P = g0[..., :3]
    covered = (app.mDepthStencilBuffer & 0xFFFFFF) < 0xFFFFFF
    coverage = {}
    for name, decals in sets.items():
        hit = torch.zeros((H, W), dtype=torch.bool, device=g0.device)
        for d in decals:
            iw = torch.tensor(list(d.invWorld), dtype=torch.float32, device=g0.device).reshape(3, 4)
            q = (P @ iw[:, :3].T + iw[:, 3]).abs()
            hit |= (q <= 0.5).all(-1)
        coverage[name] = round(float((hit & covered).float().mean().item()), 5)

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), g0.data_ptr(), nbytes, 3, stream.cuda_stream) != 0:      # 3 = hipMemcpyDeviceToDevice
            sys.exit("hipMemcpyAsync failed")

    def light():
        check(lib.crychic_deferred_light(ctx.handle, C.byref(app.mMainPassCB), f.g0_dev, f.g1_dev, f.g2_dev, f.depth_dev, f.ambient0_dev, maps,
                                         f.shadowDim, f.cube_dev, f.cubeDim, lit.data_ptr(), None, W, H, 0, H, 3, f.pcfSearchRadius, f.flags,
                                         stream.cuda_stream))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)              # ms

    # one Crychic per decal set would hold five copies of the planes: the sets share the app and are installed outside the timed region
    legs = list(sets) + ["memcpy", "light"]
    times = {k: [] for k in legs}
    for r in range(args.warmup + args.steps):
        for k in legs:
            for g, p in zip(app.mDeferred.mGBuffer, pristine):
                g.copy_(p)
            if k in sets:
                app.set_decals(sets[k], textures)
            torch.cuda.synchronize()
            if k in sets:
                t = timed(app.apply_decals)
            else:
                t = timed(memcpy if k == "memcpy" else light)
            if r >= args.warmup:
                times[k].append(t)
    med = statistics.median
    out = {"metric": "decals", "device": ctx.device_name, "frame": [W, H], "g0_plane_bytes": nbytes, "runs": args.steps}
    for k in legs:
        out[k + "_us"] = round(1e3 * med(times[k]), 2)
        out[k + "_us_min_max"] = [round(1e3 * min(times[k]), 2), round(1e3 * max(times[k]), 2)]
    for k in sets:
        out["coverage_" + k] = coverage[k]
    # the skeleton reads every depth word and the G0 texel of every covered pixel
    skeleton_bytes = W * H * 4 + int(covered.sum().item()) * 16
    out["covered_share"] = round(float(covered.float().mean().item()), 4)
    out["skeleton_bytes_read"] = skeleton_bytes
    out["skeleton_gb_per_s"] = round(skeleton_bytes / (med(times["skeleton"]) * 1e-3) / 1e9, 1)
    out["memcpy_gb_per_s"] = round(2 * nbytes / (med(times["memcpy"]) * 1e-3) / 1e9, 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
