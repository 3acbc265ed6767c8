"""Timing of the environment capture (include/crychic_hip.h "environment capture"); prints one JSON line.

    python tools/env_capture_bench.py [--steps 50] [--warmup 5]

Legs, each the median of HIP-event times over --steps runs (torch events on the caller's stream) with the device's name:
  mips_dim256 / mips_dim1024   crychic_generate_cube_mips, full chain, of a noise cube: mips_us and GB/s on the (1 + 1/3) * 24 * dim^2
                               bytes a chain moves at the least; next to it the path it replaces, measured in this process:
                               geometry.cube_mip_chain on the host plus the upload of the chain (host_chain_ms, host clock around a
                               device synchronise), and host_over_device.
  capture_dim128 / 256 / 512   Crychic.capture_environment of the box-and-grid scene (reference materials, procedural textures) at
                               (2.5, 1.25, 2.5) with shadow_dim 1024, into a kept buffer: total_ms, and the six faces' cascade
                               producers, G-buffer producers, hot paths and the mip launches (events around each call).
  frame_4k                     the 3840 x 2160 hot path of scene.make_scene (blurCount 4, 3 directional lights) alone, and with a
                               256-texel re-capture and set_cube_map before every frame.
Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, SceneGeometry, geometry as g, scene
    if not torch.cuda.is_available():
        sys.exit("env_capture_bench.py needs a HIP device")
    ctx = Context(0)
    name = ctx.device_name
    med = lambda v: statistics.median(v)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    legs = {}
    # ---- the mip chain: device kernel against host numpy + upload
    probe_app = Crychic(ctx, 64, 64, torch.zeros((256, 256, 4), dtype=torch.uint8, device=ctx.device), scene.make_cubemap(32, ctx.device), shadow_dim=256)
    for dim in (256, 1024):
        cube = np.random.default_rng(dim).integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)
        levels = g.cube_full_levels(dim)
        chain = torch.zeros((g.cube_chain_bytes(dim, levels),), dtype=torch.uint8, device=ctx.device)
        chain[:cube.size] = torch.from_numpy(cube.reshape(-1)).to(ctx.device)
        for _ in range(args.warmup):
            probe_app.generate_cube_mips(chain, dim, levels)
        dev = [event_ms(lambda: probe_app.generate_cube_mips(chain, dim, levels)) for _ in range(args.steps)]
        ref, _ = g.cube_mip_chain(cube)
        assert np.array_equal(chain.cpu().numpy(), ref), "device chain differs from geometry.cube_mip_chain"
        host = []
        for _ in range(args.steps):
            t = time.perf_counter()
            up = torch.from_numpy(g.cube_mip_chain(cube)[0]).to(ctx.device)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t) * 1e3)
        del up
        nbytes = (1.0 + 1.0 / 3.0) * 24.0 * dim * dim
        legs["mips_dim%d" % dim] = {"device": name, "levels": levels, "launches": (levels - 1 + 5) // 6, "mips_us": round(med(dev) * 1e3, 2),
                                    "gb_per_s": round(nbytes / (med(dev) * 1e-3) / 1e9, 1), "host_chain_ms": round(med(host), 3),
                                    "host_over_device": round(med(host) / med(dev), 1), "runs": args.steps}
    del probe_app

    # ---- one capture, split by stage
    geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials(), g.procedural_textures(64))
    sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    pos, SD = (2.5, 1.25, 2.5), 1024
    W, H = 3840, 2160
    planes = scene.make_scene(W, H, shadow_dim=4096, cube_dim=256, device=str(ctx.device))
    app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=4096)
    app.load_scene(planes)
    app.blurCount, app.numDirLights, app.flags = 4, 3, LIGHT_SKY
    source = planes["cube"]

    class Stage:
        """Wraps a bound method: HIP events around every call, summed per capture."""
        def __init__(self, obj, attr):
            self.fn, self.pairs = getattr(obj, attr), []
            setattr(obj, attr, self)

        def __call__(self, *a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = self.fn(*a, **k)
            e1.record()
            self.pairs.append((e0, e1))
            return r

        def take(self):
            ms = sum(a.elapsed_time(b) for a, b in self.pairs)
            self.pairs = []
            return ms

    for dim in (128, 256, 512):
        out = torch.empty((g.cube_chain_bytes(dim, g.cube_full_levels(dim)),), dtype=torch.uint8, device=ctx.device)
        for _ in range(args.warmup):
            app.capture_environment(pos, geo, sgeo, dim=dim, shadow_dim=SD, out=out)
        torch.cuda.synchronize()
        stages = {"cascades_ms": Stage(sgeo, "DrawSceneToShadowMaps"), "gbuffer_ms": Stage(geo, "DrawNormalsDepthAndGBuffer"),
                  "hot_path_ms": Stage(app._probes[(dim, SD)], "Draw"), "mips_ms": Stage(app, "generate_cube_mips")}
        total, split = [], {k: [] for k in stages}
        for _ in range(args.steps):
            total.append(event_ms(lambda: app.capture_environment(pos, geo, sgeo, dim=dim, shadow_dim=SD, out=out)))
            for k, s in stages.items():
                split[k].append(s.take())
        for s, (obj, attr) in zip(stages.values(), ((sgeo, "DrawSceneToShadowMaps"), (geo, "DrawNormalsDepthAndGBuffer"),
                                                    (app._probes[(dim, SD)], "Draw"), (app, "generate_cube_mips"))):
            delattr(obj, attr)             # the instance attribute hid the class's method
        legs["capture_dim%d" % dim] = dict({"device": name, "shadow_dim": SD, "total_ms": round(med(total), 4), "runs": args.steps},
                                           **{k: round(med(v), 4) for k, v in split.items()})

    # ---- the main 4K frame with and without a per-frame re-capture
    dim = 256
    out = torch.empty((g.cube_chain_bytes(dim, g.cube_full_levels(dim)),), dtype=torch.uint8, device=ctx.device)

    def frame_with_capture():
        app.set_cube_map(source)                          # the source of every capture: no bounce accumulates
        chain, d, n = app.capture_environment(pos, geo, sgeo, dim=dim, shadow_dim=SD, out=out)
        app.set_cube_map(chain, d, n)
        app.Draw()

    app.set_cube_map(source)
    for _ in range(args.warmup):
        app.Draw()
    alone = [event_ms(app.Draw) for _ in range(args.steps)]
    for _ in range(args.warmup):
        frame_with_capture()
    both = [event_ms(frame_with_capture) for _ in range(args.steps)]
    hot = [event_ms(app.Draw) for _ in range(args.steps)]          # the hot path alone, the captured chain bound
    legs["frame_4k"] = {"device": name, "hot_path_ms": round(med(alone), 4), "hot_path_captured_chain_ms": round(med(hot), 4),
                        "recapture_and_hot_path_ms": round(med(both), 4), "capture_dim": dim, "runs": args.steps}
    print(json.dumps({"metric": "env_capture", "device": name, "legs": legs}))
    ctx.close()


if __name__ == "__main__":
    main()
