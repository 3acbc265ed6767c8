"""Shared helpers of the local-light tests (point lights, spot lights, shadowed spot lights): light lists, scenes, spot shadow maps
and transforms, and the C++ veneer's local-light driver (tests/cpp/local_lights_driver.cpp)."""
import ctypes as C
import math
import subprocess

import numpy as np

import oracle_lib
import scene_util

FIX_ALL = 0x100 | 0x200 | 0x400          # CRYCHIC_FIX_Q1 | Q3 | Q4 (the oracle uses the same bits)


def light_array(lights):
    from crychic_renderer_amd._lib import Light
    arr = (Light * len(lights))()
    for k, L in enumerate(lights):
        C.memmove(C.addressof(arr[k]), C.addressof(L), 48)
    return arr


def as_or_lights(lights):
    arr = (oracle_lib.OrLight * len(lights))()
    C.memmove(C.addressof(arr), C.addressof(lights), C.sizeof(arr))
    return arr


def spots_for_test(power=None):
    """A ring aimed at the box field plus irregular members: an unnormalised direction, a light aimed away from everything,
    one that reaches nothing, one that reaches everything.  power: override every SpotPower."""
    from crychic_renderer_amd import scene
    L = scene.spot_light_ring(12, radius=10.0, y=6.0, falloff_end=25.0, spot_power=8.0)
    L[1].Direction[:] = [2.0 * v for v in L[1].Direction]          # used as given: a longer vector sharpens the cone
    L[2].Direction[:] = (0.0, 1.0, 0.0)                             # aimed at the sky: only the 0.001 floor lights
    L[3].Position[:] = (500.0, 500.0, 500.0)                        # reaches nothing
    L[4].FalloffEnd = 300.0; L[4].SpotPower = 64.0                  # reaches everything, tight cone
    L[5].Strength[:] = (3.0, 0.3, 0.2); L[5].SpotPower = 1.0
    L[6].FalloffStart = 0.5; L[6].SpotPower = 200.0
    if power is not None:
        for k in range(len(L)):
            L[k].SpotPower = power
    return L


def points_for_test():
    from crychic_renderer_amd import scene
    L = scene.point_light_grid(4)
    L[2].Strength[:] = (0.2, 2.5, 0.3)
    return L


def _cpu(W, H):
    """The CPU scene: (planes as built, numpy planes, constants, the oracle's view of the pass constants)."""
    pl = scene_util.cpu_scene(W, H, 256, 32)
    p = scene_util.np_planes(pl)
    c = pl["consts"]
    return pl, p, c, oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)


def spot_transforms(spots, count, fov_y=0.5 * math.pi, z_near=0.5):
    """The product's crychic_update_spot_shadow_transform of the first `count` lights: (views, projs, transforms), untransposed."""
    from crychic_renderer_amd import lib
    out = []
    for k in range(count):
        lv, lp, st = ((C.c_float * 16)() for _ in range(3))
        assert lib.crychic_update_spot_shadow_transform(C.byref(spots[k]), fov_y, z_near, lv, lp, st) == 0
        out.append(tuple(np.asarray(m[:], np.float32).reshape(4, 4) for m in (lv, lp, st)))
    return out


def with_transforms(pass_cb, Ts):
    """Copies of the product's pass constants (and the oracle's view of them) with ShadowTransforms[4 + k] = Ts[k] (stored
    transposed: Ts are given as 16 floats already in that layout)."""
    from crychic_renderer_amd._lib import PassConstants
    cb = PassConstants.from_buffer_copy(pass_cb)
    for k, T in enumerate(Ts):
        cb.ShadowTransforms[4 + k][:] = [float(v) for v in np.asarray(T, np.float32).reshape(-1)]
    return cb, oracle_lib.as_oracle_cb(cb, oracle_lib.OrPassConstants)


def transposed(st):
    return st.T.reshape(-1).copy()


def random_maps(count, dim, seed):
    """D24 maps with occluders: depths in [0.85, 1) with square blocks at 1 (lit) and at 0.5 (occluders in front)."""
    rng = np.random.default_rng(seed)
    m = (rng.uniform(0.85, 1.0, (count, dim, dim)) * 16777215.0).astype(np.uint32)
    for k in range(count):
        for _ in range(6):
            x, y, s = rng.integers(0, dim, 3)
            m[k, y:y + s // 3 + 1, x:x + s // 3 + 1] = rng.choice([0x00FFFFFF, 0x007FFFFF])
    return m | (rng.integers(0, 256, m.shape, dtype=np.uint32) << 24)          # the X8 byte is ignored


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------

def _device_scene(ctx, W, H, SD=256, CD=32):
    import torch
    pl = scene_util.cpu_scene(W, H, SD, CD)
    p = scene_util.np_planes(pl)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).to(ctx.device)
           for k, v in p.items()}
    return pl, p, dev


def _dev_lights(ctx, lights):
    import torch
    if lights is None:
        return None, 0
    return torch.from_numpy(np.frombuffer(bytes(lights), np.uint8).copy()).to(ctx.device), len(lights)


dev_lights = _dev_lights          # for library modules


def _app(ctx, W, H, dev, c, blur=3, ndl=3):
    from crychic_renderer_amd import Crychic, LIGHT_SKY
    app = Crychic(ctx, W, H, dev["randvec"], dev["cube"], shadow_dim=256)
    app.load_scene({**dev, "consts": c})
    app.blurCount, app.numDirLights, app.flags = blur, ndl, LIGHT_SKY
    return app


# The veneer driver's frame: 128 x 96, cascades 256, cube 32, blurCount 3, three directional lights; 3 shadowed maps of 128.
DRIVER_FRAME = dict(W=128, H=96, SD=256, CD=32, BC=3, NL=3, COUNT=3, DIM=128)


def run_local_lights_driver(d):
    """Writes the driver's inputs into directory `d` (the planes veneer_driver reads, randvec.bin, points.bin, spots.bin,
    spotmap<k>.bin and scene_spots.bin), runs tests/cpp/local_lights_driver and returns (planes as built, numpy planes, points,
    spots, maps)."""
    import test_cpp_veneer
    from crychic_renderer_amd import scene
    exe = test_cpp_veneer.build_driver("local_lights_driver")
    F = DRIVER_FRAME
    pl = scene_util.cpu_scene(F["W"], F["H"], F["SD"], F["CD"])
    p = scene_util.np_planes(pl)
    p["depth"].tofile(d + "/depth.bin"); p["normal"].tofile(d + "/normal.bin"); p["cube"].tofile(d + "/cube.bin")
    p["randvec"].tofile(d + "/randvec.bin")
    for i in range(3):
        p["g%d" % i].tofile(d + "/g%d.bin" % i)
    for i in range(4):
        p["shadow"][i].tofile(d + "/shadow%d.bin" % i)
    points, spots = points_for_test(), spots_for_test()
    open(d + "/points.bin", "wb").write(bytes(points))
    open(d + "/spots.bin", "wb").write(bytes(spots))
    open(d + "/scene_spots.bin", "wb").write(bytes(scene.shadow_spot_lights(1)))
    maps = random_maps(F["COUNT"], F["DIM"], 21)
    for k in range(F["COUNT"]):
        maps[k].tofile(d + "/spotmap%d.bin" % k)
    r = subprocess.run([exe, d] + [str(F[k]) for k in ("W", "H", "SD", "CD", "BC", "NL", "COUNT", "DIM")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "local lights driver ok" in r.stdout
    return pl, p, points, spots, maps
