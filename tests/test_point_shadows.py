"""Shadowed point lights (extension, include/crychic_hip.h crychic_deferred_light_point_shadows): cube shadows for the first four
point lights, six D24 faces each, read through one projection per light and an exact permutation of v = pos - Position.  Parity is
against this repo's checker (tests/point_shadow_ref/point_shadow_ref.c, which includes tests/local_light_ref/local_light_ref.c
unchanged).  The checker is anchored to the existing shadowed-spot checker (a projection with s = 1), to a float64 restatement of the
factor, and to the CPU oracle rasteriser's geometry (a box's shadow across a face boundary)."""
import ctypes as C
import math

import numpy as np
import pytest

import hostsim_lib
import local_light_lib
import oracle_lib
import point_shadow_lib
from point_shadow_lib import point_desc as _point_desc, point_transforms, random_cubes, spot_desc as _spot_desc  # noqa: F401 (other test modules import them from here)
from local_lights_util import (FIX_ALL, _app, _cpu, _dev_lights, _device_scene, light_array, points_for_test, random_maps,
                               spot_transforms, spots_for_test, transposed, with_transforms)

CENTRE_P = np.zeros(16, np.float32)          # untransposed: every position -> face centre (0.5, 0.5) at depth 0, s = 1
CENTRE_P[12], CENTRE_P[13], CENTRE_P[15] = 0.5, 0.5, 1.0
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
UPS = np.array([[0, 1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1], [0, 1, 0], [0, 1, 0]], np.float64)


def shadowed_points():
    """Four point lights above boxes of the reference scene, then the grid of points_for_test."""
    from crychic_renderer_amd import scene
    return light_array(list(scene.shadow_point_lights(4)) + list(points_for_test()))


def _mul_f32(p, V):
    """mul(float4(p, 1), V) in float32, the products summed in order."""
    f = np.float32
    return [((f(p[0]) * V[0, j] + f(p[1]) * V[1, j]) + f(p[2]) * V[2, j]) + V[3, j] for j in range(3)]


def _same_up_to_zero_sign(a, b):
    a, b = np.float32(a), np.float32(b)
    return a.view(np.uint32) == b.view(np.uint32) or (a == 0 and b == 0)


# ---- CPU tier: the face step and the builder ---------------------------------------------------------------------------------

def test_face_table_is_the_builders_look_at(built_lib):
    """For random lights and positions, mul(float4(pos, 1), lightView[f]) of the builder equals the face table's (a, b, c) bit for
    bit up to the sign of zero, in the checker and in the product body; the selected face is the one with c == max |v|."""
    from crychic_renderer_amd._lib import Light
    rng = np.random.default_rng(3)
    ps = point_shadow_lib.load()
    n = 0
    for trial in range(40):
        L = Light()
        L.Position[:] = [float(x) for x in rng.uniform(-50, 50, 3).astype(np.float32)]
        L.FalloffStart, L.FalloffEnd = 1.0, float(rng.uniform(5, 40))
        views = point_transforms([L], 1, int(rng.choice([16, 512])))[0][0]
        lp = np.asarray(L.Position[:], np.float32)
        for _ in range(50):
            pos = (lp + rng.uniform(-30, 30, 3) * rng.choice([1.0, 1e-3], 3)).astype(np.float32)
            if trial % 5 == 0:                                      # exact ties between components
                pos[1] = lp[1] + (pos[0] - lp[0]) * rng.choice([1, -1])
            v = (pos - lp).astype(np.float32)
            f, abc = ps.face(v)
            fh, abch = hostsim_lib.load().point_face(v)
            assert f == fh and abc.view(np.uint32).tolist() == abch.view(np.uint32).tolist()
            got = _mul_f32(pos, views[f])
            for c in range(3):
                assert _same_up_to_zero_sign(got[c], abc[c]), (f, pos, got, abc)
            assert abc[2] == np.abs(v).max() and abc[2] >= 0
            n += 1
    assert n == 2000


def _look_at_f64(eye, axis, up):
    z = axis / np.linalg.norm(axis)
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    V = np.zeros((4, 4))
    V[:3, 0], V[:3, 1], V[:3, 2] = x, y, z
    V[3, :3] = (-x @ eye, -y @ eye, -z @ eye)
    V[3, 3] = 1.0
    return V


def test_builder_matches_float64(built_lib):
    """crychic_update_point_shadow_transforms == LookAtLH(Position, Position + axis_f, up_f) and PerspectiveFovLH with
    xScale = yScale = (dim - 4) / dim, aspect 1, zNear .. FalloffEnd, and lightProj * T, in float64; every point of a face's
    90-degree region projects to texel coordinates in [2, dim - 2]."""
    tex = np.array([[0.5, 0, 0, 0], [0, -0.5, 0, 0], [0, 0, 1, 0], [0.5, 0.5, 0, 1]])
    lights = shadowed_points()
    for dim, zn in ((16, 0.5), (17, 0.1), (1024, 2.0)):
        for k, (views, lp, sp) in enumerate(point_transforms(lights, 6, dim, zn)):
            L = lights[k]
            pos = np.asarray(L.Position[:], np.float64)
            s = (dim - 4) / dim
            P = np.zeros((4, 4)); P[0, 0] = P[1, 1] = s; P[2, 2] = L.FalloffEnd / (L.FalloffEnd - zn); P[2, 3] = 1.0
            P[3, 2] = -zn * L.FalloffEnd / (L.FalloffEnd - zn)
            for f in range(6):
                V = _look_at_f64(pos, AXES[f], UPS[f])
                assert np.abs(views[f] - V).max() <= 1e-6 * max(1.0, np.abs(V).max()), (dim, k, f)
            assert np.abs(lp - P).max() <= 1e-6 and np.abs(sp - P @ tex).max() <= 1e-6
            for a, b in ((1, 1), (-1, 1), (1, -1), (-1, -1), (0, 0), (1, 0)):
                q = np.array([a * 3.0, b * 3.0, 3.0, 1.0]) @ sp.astype(np.float64)
                tx, ty = q[0] / q[3] * dim, q[1] / q[3] * dim
                assert 2 - 1e-4 <= tx <= dim - 2 + 1e-4 and 2 - 1e-4 <= ty <= dim - 2 + 1e-4


def test_builder_argument_errors(built_lib):
    """NULL pointers, dim outside 16 .. 16384, zNear <= 0, zNear >= FalloffEnd and a non-finite Position are CRYCHIC_E_INVALID_ARG."""
    from crychic_renderer_amd import lib
    L = shadowed_points()[0]
    lv, lp, sp = ((C.c_float * 16) * 6)(), (C.c_float * 16)(), (C.c_float * 16)()
    call = lambda light, dim=64, zn=0.5, m=(lv, lp, sp): lib.crychic_update_point_shadow_transforms(light, dim, zn, *m)
    assert call(C.byref(L)) == 0
    for dim in (0, 15, 16385):
        assert call(C.byref(L), dim=dim) == -1, dim
    assert call(C.byref(L), dim=16) == 0 and call(C.byref(L), dim=16384) == 0
    for zn in (0.0, -1.0, L.FalloffEnd, L.FalloffEnd + 1.0, float("nan")):
        assert call(C.byref(L), zn=zn) == -1, zn
    for bad in (float("inf"), float("nan")):
        B = light_array([L])[0]
        B.Position[1] = bad
        assert call(C.byref(B)) == -1
    assert call(None) == -1
    for m in ((None, lp, sp), (lv, None, sp), (lv, lp, None)):
        assert call(C.byref(L), m=m) == -1


# ---- CPU tier: the checker's anchors ------------------------------------------------------------------------------------------

def _edge_positions(lp, rng, reach):
    """Positions around a light: face edges and corners (|v.x| = |v.y| = |v.z|) and random directions, at distances up to `reach`."""
    out = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                for t in (0.7, 0.25 * reach, 0.5 * reach):
                    out.append(lp + np.array([sx, sy, sz]) * t)                   # corners
                    out.append(lp + np.array([sx * t, sy * t, 0.3 * t * sz]))     # edges
                    out.append(lp + np.array([0.0, sy * t, sz * t]))
    for _ in range(300):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        out.append(lp + d * rng.uniform(0.6, 0.95 * reach / math.sqrt(3)) * np.sqrt(3))
    return [np.asarray(p, np.float32) for p in out if np.linalg.norm(p - lp) <= 0.95 * reach]


@pytest.mark.parametrize("dim", [16, 17, 1024])
def test_no_seams_cleared_maps(built_lib, dim):
    """Faces cleared to 0xFFFFFF: s == 1.0f exactly at in-range positions, face edges and corners included, in the checker and the
    product body; with xScale = 1 (exact 90-degree faces) some boundary position reads the border and fails."""
    ps = point_shadow_lib.load()
    rng = np.random.default_rng(dim)
    faces = np.full((6, dim, dim), 0xFFFFFF, np.uint32)
    lights = shadowed_points()
    failed = 0
    for k, (_, _, sp) in enumerate(point_transforms(lights, 4, dim)):
        lp = np.asarray(lights[k].Position[:], np.float32)
        narrow = sp.copy()
        narrow[0, 0], narrow[1, 1] = 0.5, -0.5                   # lightProj with xScale = yScale = 1, times T
        for pos in _edge_positions(lp, rng, lights[k].FalloffEnd):
            assert ps.factor(faces, sp, lp, pos) == 1.0, (dim, k, pos)
            assert hostsim_lib.load().point_shadow_factor(faces, sp, lp, pos) == 1.0, (dim, k, pos)
            failed += ps.factor(faces, narrow, lp, pos) < 1.0
    assert failed > 0


def test_no_seams_frame(built_lib):
    """Cleared faces give the frame without point shadows bit for bit (checker and product body)."""
    W, H = 96, 64
    _, p, c, pcb = _cpu(W, H)
    ps = point_shadow_lib.load()
    points = shadowed_points()
    cubes = np.full((4, 6, 32, 32), 0xFFFFFF, np.uint32)
    projs = [sp.reshape(-1) for _, _, sp in point_transforms(points, 4, 32)]
    for which, fn, cb in (("checker", ps.checker, pcb), ("host", hostsim_lib.load().light_frame, c.pass_cb)):
        base, rbase = fn(cb, p, None, 3, 0.0, 1, points=points)
        got, rgot = fn(cb, p, None, 3, 0.0, 1, points=points, cubes=cubes, projs=projs)
        assert np.array_equal(got, base) and np.array_equal(rgot.view(np.uint32), rbase.view(np.uint32)), which


def _segment_hits_box(a, b, lo, hi):
    """Float64 slab test: does the segment a -> b meet the closed box [lo, hi]?"""
    t0, t1 = 0.0, 1.0
    d = b - a
    for i in range(3):
        if abs(d[i]) < 1e-12:
            if not lo[i] <= a[i] <= hi[i]:
                return False
            continue
        u, w = (lo[i] - a[i]) / d[i], (hi[i] - a[i]) / d[i]
        t0, t1 = max(t0, min(u, w)), min(t1, max(u, w))
        if t0 > t1:
            return False
    return True


def test_geometry_anchor_or_raster(built_lib, oracle):
    """The CPU oracle rasteriser renders the six faces of one light over the grid and one box (dim 256); the box's shadow on the grid
    crosses the boundary between the -Y and -X faces.  At ground points whose 3-texel neighbourhood on their face agrees, the checker
    gives s == 0 where the float64 segment from the point to the light meets the box and s == 1 where it does not."""
    from crychic_renderer_amd import geometry as g
    from crychic_renderer_amd._lib import Light
    dim, zn = 256, 0.5
    box = g.create_box(1.0, 1.0, 1.0, 3)
    grid = g.create_grid(20.0, 30.0, 60, 40)
    items = [(box[0], box[1], g.make_instances([g.world_matrix((1.6, 1.6, 1.6), (0.0, 0.8, 0.0))], [0])),
             (grid[0], grid[1], g.make_instances([g.world_matrix((3.0, 3.0, 3.0))], [1]))]
    L = Light()
    L.Position[:] = (1.0, 3.0, 0.7)
    L.FalloffStart, L.FalloffEnd = 1.0, 12.0
    views, lp, sp = point_transforms([L], 1, dim, zn)[0]
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    faces = np.stack([oracle_lib.rasterize(oracle, 0, eye, (views[f] @ lp).astype(np.float32).T.reshape(-1), items, None, None, dim, dim,
                                           10000, 2.0)["depth"] for f in range(6)])
    ps = point_shadow_lib.load()
    light = np.asarray(L.Position[:], np.float64)
    lo, hi = np.array([-0.8, 0.0, -0.8]), np.array([0.8, 1.6, 0.8])
    inv_views = [np.linalg.inv(views[f].astype(np.float64)) for f in range(6)]
    scale = (dim - 4) / dim

    def ground_of_texel(f, tx, ty):
        x, y = (tx / dim) * 2 - 1, 1 - (ty / dim) * 2
        dv = np.array([x / scale, y / scale, 1.0, 0.0]) @ inv_views[f]
        if dv[1] >= -1e-9:
            return None
        return light + dv[:3] * (-light[1] / dv[1])

    counts = {0.0: 0, 1.0: 0}
    faces_hit = set()
    for x in np.linspace(-6.0, 6.0, 61):
        for z in np.linspace(-6.0, 6.0, 61):
            pos = np.array([x, 0.0, z], np.float32)
            if np.linalg.norm(pos - light) > 0.95 * L.FalloffEnd:
                continue
            f, abc = ps.face((pos - light.astype(np.float32)).astype(np.float32))
            q = np.append(abc.astype(np.float64), 1.0) @ sp.astype(np.float64)
            tx, ty = q[0] / q[3] * dim, q[1] / q[3] * dim
            hits = set()
            for ox in (-3, 0, 3):
                for oy in (-3, 0, 3):
                    gp = ground_of_texel(f, tx + ox, ty + oy)
                    hits.add(None if gp is None else _segment_hits_box(gp, light, lo, hi))
            if len(hits) != 1 or None in hits:
                continue
            s = ps.factor(faces, sp, light, pos)
            want = 0.0 if hits.pop() else 1.0
            assert s == want, (pos, f, s, want)
            counts[want] += 1
            if want == 0.0:
                faces_hit.add(f)
    assert counts[0.0] > 40 and counts[1.0] > 400, counts
    assert {1, 3} <= faces_hit, faces_hit                        # the shadow lies on the -X and the -Y face


def _factor_f64(faces, sp, light, pos):
    """Float64 restatement: the face of the float32 v, the projection and the nine gsamShadow taps in float64."""
    dim = faces.shape[1]
    v = (np.asarray(pos, np.float32) - np.asarray(light, np.float32)).astype(np.float32)
    ax = np.abs(v)
    axis = 0 if ax[0] >= ax[1] and ax[0] >= ax[2] else (1 if ax[1] >= ax[2] else 2)
    neg = not v[axis] >= 0
    f = 2 * axis + int(neg)
    x, y, z = (float(t) for t in v)
    abc = [(-z, y, x), (z, y, -x), (x, -z, y), (x, z, -y), (x, y, z), (-x, y, -z)][f]
    d = (faces[f] & 0xFFFFFF).astype(np.float64) / 16777215.0
    q = np.append(np.asarray(abc, np.float64), 1.0) @ np.asarray(sp, np.float64)
    u, w, depth = q[0] / q[3], q[1] / q[3], q[2] / q[3]
    dx = 1.0 / dim
    tot = 0.0
    for oy in (-dx, 0.0, dx):
        for ox in (-dx, 0.0, dx):
            tx, ty = (u + ox) * dim - 0.5, (w + oy) * dim - 0.5
            i0, j0 = math.floor(tx), math.floor(ty)
            fx, fy = tx - i0, ty - j0

            def cmp(i, j):
                t = d[j, i] if 0 <= i < dim and 0 <= j < dim else 0.0
                return 1.0 if depth <= t else 0.0
            tot += (cmp(i0, j0) * (1 - fx) + cmp(i0 + 1, j0) * fx) * (1 - fy) + (cmp(i0, j0 + 1) * (1 - fx) + cmp(i0 + 1, j0 + 1) * fx) * fy
    return tot / 9.0


def test_checker_factor_matches_float64_restatement(built_lib):
    """Random faces and positions around the lights: the checker's factor is the float64 restatement's within 1e-5 and exact where
    that gives 0 or 1; the product body's equals the checker's bit for bit."""
    rng = np.random.default_rng(5)
    ps = point_shadow_lib.load()
    lights = shadowed_points()
    diffs, partial = [], 0
    for k, (_, _, sp) in enumerate(point_transforms(lights, 4, 64)):
        for dim in (64,):
            faces = random_cubes(1, dim, 40 + k)[0]
            lp = np.asarray(lights[k].Position[:], np.float32)
            for _ in range(150):
                d = rng.normal(size=3); d /= np.linalg.norm(d)
                pos = (lp + d * rng.uniform(1.0, 0.9 * lights[k].FalloffEnd)).astype(np.float32)
                s = ps.factor(faces, sp, lp, pos)
                assert np.float32(s).view(np.uint32) == np.float32(hostsim_lib.load().point_shadow_factor(faces, sp, lp, pos)).view(np.uint32)
                ref = _factor_f64(faces, sp, lp, pos)
                diffs.append(abs(s - ref))
                if ref in (0.0, 1.0):
                    assert s == ref
                else:
                    partial += 1
    assert max(diffs) < 1e-5, max(diffs)
    assert partial > 20


@pytest.mark.parametrize("spot_count", [0, 3])
def test_checker_centre_projection_is_the_spot_checker(spot_count):
    """A shadowProj that sends every point to the face centre at depth 0 gives ss_deferred_light_spots_shadowed's frame bit for bit."""
    W, H = 96, 64
    _, p, c, _ = _cpu(W, H)
    spots, points = spots_for_test(), shadowed_points()
    cb, pcb = with_transforms(c.pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 8)])
    maps = random_maps(spot_count, 32, 3) if spot_count else None
    ref, rref = local_light_lib.load().checker(pcb, p, None, 3, 0.0, 1 | FIX_ALL, points=points, spots=spots, maps=maps)
    got, rgot = point_shadow_lib.load().checker(pcb, p, None, 3, 0.0, 1 | FIX_ALL, points=points, spots=spots, maps=maps,
                                                cubes=random_cubes(4, 32, 9), projs=[CENTRE_P] * 4)
    assert np.array_equal(got, ref) and np.array_equal(rgot.view(np.uint32), rref.view(np.uint32))


def _frame_setup(W, H, count, dim, spot_count, seed=1):
    pl, p, c, _ = _cpu(W, H)
    spots, points = spots_for_test(), shadowed_points()
    cb, pcb = with_transforms(c.pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 8)])
    maps = random_maps(spot_count, 48, seed) if spot_count else None
    cubes = random_cubes(count, dim, seed + 7)
    projs = [sp.reshape(-1) for _, _, sp in point_transforms(points, count, dim)]
    return p, cb, pcb, spots, points, maps, cubes, projs


@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("count,spot_count", [(1, 0), (2, 3), (4, 0), (4, 3)])
def test_kernel_body_matches_checker(built_lib, chain, count, spot_count):
    """light_core.hpp's body (pbr_point_light with PointShadowOf, built for the host) equals the checker bit for bit: point shadow
    counts 1, 2 and 4, spot shadow counts 0 and 3, Q fixes off and on, both PCF radii, with and without the cube chain."""
    from crychic_renderer_amd import geometry as g
    W, H = 98, 66
    p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, count, 48, spot_count, seed=count)
    kw, extra = {}, 0
    if chain:
        cube, levels = g.cube_mip_chain(p["cube"])
        p = dict(p, cube=cube)
        kw, extra = dict(cube_dim=32), (levels & 15) << 16
    ps = point_shadow_lib.load()
    for fixes, ndl, radius in ((0, 1, 0.0), (FIX_ALL, 3, 0.01)):
        flags = fixes | 1 | extra
        args = dict(points=points, spots=spots, maps=maps, cubes=cubes, projs=projs, **kw)
        got, grad = hostsim_lib.load().light_frame(cb, p, None, ndl, radius, flags, **args)
        ref, rref = ps.checker(pcb, p, None, ndl, radius, flags, **args)
        assert np.array_equal(got, ref) and np.array_equal(grad.view(np.uint32), rref.view(np.uint32)), fixes
        base, _ = ps.checker(pcb, p, None, ndl, radius, flags, points=points, spots=spots, maps=maps, **kw)
        assert (ref != base).any()                                           # the point shadows change the frame


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------

def _light(lib, ctx, cb, dev, W, H, flags, points, spots, sdesc, pdesc, ndl=3, radius=0.0, ambient=None, row0=0, rows=None, out=None,
           rad=None, cube=None, entry="point_shadows", shadow_dim=256, cube_dim=32):
    """One crychic_deferred_light_point_shadows / _spots_shadowed / _spots call (entry "point_shadows" / "spots_shadowed" / "spots")
    on the planes of dev; shadow_dim / cube_dim: the sizes of dev's cascades and cube map."""
    import torch
    from crychic_renderer_amd.renderer import _ptr, _stream
    rows = H - row0 if rows is None else rows
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev["g0"].device) if out is None else out
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=dev["g0"].device) if rad is None else rad
    sh = (C.c_void_p * 4)(*[dev["shadow"][k].data_ptr() for k in range(4)])
    args = [ctx.handle, C.byref(cb), _ptr(dev["g0"]), _ptr(dev["g1"]), _ptr(dev["g2"]), _ptr(dev["depth"]), _ptr(ambient), sh, shadow_dim,
            _ptr(cube if cube is not None else dev["cube"]), cube_dim, _ptr(out), _ptr(rad), W, H, row0, rows, ndl, radius, flags,
            _ptr(points[0]), points[1], _ptr(spots[0]), spots[1], None if sdesc is None else C.byref(sdesc)]
    if entry == "point_shadows":
        rc = lib.crychic_deferred_light_point_shadows(*args, None if pdesc is None else C.byref(pdesc), _stream(ctx.device))
    elif entry == "spots":
        rc = lib.crychic_deferred_light_spots(*args[:-1], _stream(ctx.device))
    else:
        rc = lib.crychic_deferred_light_spots_shadowed(*args, _stream(ctx.device))
    return rc, out, rad


def _produce_cubes(ctx, lights, count, dim, z_near=0.5):
    """The six faces of the first `count` lights rendered from the reference scene's shadow casters, 12 faces per call."""
    import torch
    from crychic_renderer_amd import SceneGeometry, geometry as g
    from crychic_renderer_amd._lib import PassConstants
    sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
    cubes = torch.full((count, 6, dim, dim), 0xFFFFFF, dtype=torch.int32, device=ctx.device)
    tr = point_transforms(lights, count, dim, z_near)
    cbs, planes = [], []
    for k, (views, lp, _) in enumerate(tr):
        for f in range(6):
            cb = PassConstants(); cb.ViewProj[:] = list((views[f] @ lp).astype(np.float32).T.reshape(-1))
            cbs.append(cb); planes.append(cubes[k, f])
    for i in range(0, len(cbs), 12):
        sgeo.DrawSceneToShadowMaps(cbs[i:i + 12], planes[i:i + 12])
    return cubes, [sp.reshape(-1) for _, _, sp in tr]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(322, 190), (1920, 1080)])
def test_deferred_light_point_shadows_on_device(built_lib, W, H):
    """crychic_deferred_light_point_shadows == the checker bit for bit (RGBA8 and radiance) with 4 point shadows and 3 spot shadows,
    faces from the producer: both PCF radii, Q fixes off and on, with and without the ambient map."""
    import torch
    from crychic_renderer_amd import Context
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    ps = point_shadow_lib.load()
    points, spots = shadowed_points(), spots_for_test()
    dp, ds = _dev_lights(ctx, points), _dev_lights(ctx, spots)
    rng = np.random.default_rng(11)
    ao = rng.integers(20000, 65535, (H // 2, W // 2), dtype=np.uint16)
    ao_dev = torch.from_numpy(ao.view(np.int16)).to(ctx.device)
    cb, pcb = with_transforms(pl["consts"].pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 8)])
    maps = random_maps(3, 128, 5)
    mdev = torch.from_numpy(maps.view(np.int32)).to(ctx.device)
    cubes_dev, projs = _produce_cubes(ctx, points, 4, 256)
    torch.cuda.synchronize()
    cubes = cubes_dev.cpu().numpy().view(np.uint32)
    assert (cubes < 0xFFFFFF).any()
    for fixes, radius, with_ao in ((0, 0.0, False), (FIX_ALL, 0.01, True)):
        rc, out, rad = _light(built_lib.lib, ctx, cb, dev, W, H, 1 | fixes, dp, ds, _spot_desc(mdev), _point_desc(cubes_dev, projs),
                              radius=radius, ambient=ao_dev if with_ao else None)
        built_lib.check(rc)
        torch.cuda.synchronize()
        a = ao if with_ao else None
        ref, rref = ps.checker(pcb, p, a, 3, radius, 1 | fixes, points=points, spots=spots, maps=maps, cubes=cubes, projs=projs)
        assert np.array_equal(out.cpu().numpy(), ref), fixes
        assert np.array_equal(rad.cpu().numpy().view(np.uint32), rref.view(np.uint32)), fixes
    ctx.close()


@pytest.mark.gpu
def test_point_shadows_cube_chain_row_ranges(built_lib):
    """With the cube map's mip chain: the frame lit as even row ranges == the checker."""
    import torch
    from crychic_renderer_amd import Context, geometry as g
    W, H = 200, 120
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    points = shadowed_points()
    chain, levels = g.cube_mip_chain(p["cube"])
    chain_dev = torch.from_numpy(chain).to(ctx.device)
    flags = 1 | ((levels & 15) << 16)
    cubes = random_cubes(2, 64, 2)
    projs = [sp.reshape(-1) for _, _, sp in point_transforms(points, 2, 64)]
    cdev = torch.from_numpy(cubes.view(np.int32)).to(ctx.device)
    dp = _dev_lights(ctx, points)
    cb = pl["consts"].pass_cb
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    for r0, rn in ((0, 36), (36, 50), (86, 34)):
        built_lib.check(_light(built_lib.lib, ctx, cb, dev, W, H, flags, dp, (None, 0), None, _point_desc(cdev, projs), row0=r0, rows=rn,
                               out=out, rad=rad, cube=chain_dev)[0])
    torch.cuda.synchronize()
    pcb = oracle_lib.as_oracle_cb(cb, oracle_lib.OrPassConstants)
    ref, rref = point_shadow_lib.load().checker(pcb, dict(p, cube=chain), None, 3, 0.0, flags, points=points, cubes=cubes, projs=projs,
                                                cube_dim=32)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(rad.cpu().numpy().view(np.uint32), rref.view(np.uint32))
    ctx.close()


@pytest.mark.gpu
def test_point_shadow_identities(built_lib):
    """Against the _spots_shadowed entry: a NULL descriptor and count 0 are bit-identical (with and without spot lights and spot
    shadows); cleared faces give the unshadowed frame."""
    import torch
    from crychic_renderer_amd import Context
    W, H = 256, 144
    lib = built_lib.lib
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    points, spots = shadowed_points(), spots_for_test()
    dp, ds = _dev_lights(ctx, points), _dev_lights(ctx, spots)
    cb, _ = with_transforms(pl["consts"].pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 8)])
    mdev = torch.from_numpy(random_maps(3, 64, 9).view(np.int32)).to(ctx.device)
    cdev = torch.from_numpy(random_cubes(4, 32, 4).view(np.int32)).to(ctx.device)
    projs = [sp.reshape(-1) for _, _, sp in point_transforms(points, 4, 32)]

    def frame(spots_dev, sdesc, pdesc, entry="point_shadows"):
        rc, out, rad = _light(lib, ctx, cb, dev, W, H, 1, dp, spots_dev, sdesc, pdesc, radius=0.01, entry=entry)
        built_lib.check(rc)
        torch.cuda.synchronize()
        return out.cpu().numpy(), rad.cpu().numpy().view(np.uint32)

    for spots_dev, sdesc in ((ds, _spot_desc(mdev)), (ds, None), ((None, 0), None)):
        plain = frame(spots_dev, sdesc, None, entry="spots_shadowed")
        for pdesc in (None, _point_desc(None), _point_desc(cdev, projs, count=0)):
            got = frame(spots_dev, sdesc, pdesc)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        shadowed = frame(spots_dev, sdesc, _point_desc(cdev, projs))
        assert not np.array_equal(shadowed[0], plain[0])
        cleared = torch.full_like(cdev, 0xFFFFFF)
        got = frame(spots_dev, sdesc, _point_desc(cleared, projs))
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    ctx.close()


@pytest.mark.gpu
def test_hot_path_point_shadows_whole_strips_and_shared(built_lib, oracle):
    """Crychic.set_point_shadows: crychic_draw_hot_path_point_shadows == the checker fed the oracle's ambient map; strips == the whole
    frame; crychic_draw_hot_path_shared_point_shadows at one rank (1 and 3 parts) == the single-GPU frame; count 0 through the new
    entries == the _spots_shadowed entries."""
    import torch
    from crychic_renderer_amd import Context, sharding
    from crychic_renderer_amd.renderer import _ptr, _stream
    W, H = 256, 144
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    app = _app(ctx, W, H, dev, c)
    points, spots = shadowed_points(), spots_for_test()
    app.set_point_lights(points)
    app.set_spot_lights(spots)
    app.set_spot_shadows(3, dim=128)
    smaps = random_maps(3, 128, 4)
    app.mSpotShadowMaps.copy_(torch.from_numpy(smaps.view(np.int32)))
    app.set_point_shadows(4, dim=64)
    cubes = random_cubes(4, 64, 6)
    app.mPointShadowMaps.copy_(torch.from_numpy(cubes.view(np.int32)))
    app.Draw()
    torch.cuda.synchronize()
    full = app.mBackBuffer.cpu().numpy().copy()
    ao = oracle.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)
    _, pcb = with_transforms(c.pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 3)])
    projs = [sp.reshape(-1) for _, _, sp in point_transforms(points, 4, 64)]
    ref, _ = point_shadow_lib.load().checker(pcb, p, ao, 3, app.pcfSearchRadius, 1, points=points, spots=spots, maps=smaps, cubes=cubes,
                                             projs=projs)
    assert np.array_equal(full, ref)
    app.mBackBuffer.zero_()
    for rank in range(3):
        r0, rn = C.c_uint32(), C.c_uint32()
        built_lib.check(built_lib.lib.crychic_strip_rows(H, 3, rank, C.byref(r0), C.byref(rn)))
        app.Draw(r0.value, rn.value)
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), full)
    ex = sharding.StripExchange(ctx, W, H, 1, 0, sharding.StripExchange.new_unique_id(), slots=1)
    for parts in (1, 3):
        app.mBackBuffer.zero_()
        app.Draw(shared=(ex.handle, None, parts))
        torch.cuda.synchronize()
        assert np.array_equal(app.mBackBuffer.cpu().numpy(), full), parts
    f = app.frame_desc()
    lib = built_lib.lib
    sd = app._spotShadow[0]
    cbT = with_transforms(c.pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 3)])[0]
    frames = []
    for entry in ("spots_shadowed", "point_shadows", "shared_spots_shadowed", "shared_point_shadows"):
        app.mBackBuffer.fill_(3)
        a = (C.byref(app.mSsaoCB), C.byref(cbT), C.byref(f))
        n = len(spots)
        if entry == "spots_shadowed":
            built_lib.check(lib.crychic_draw_hot_path_spots_shadowed(ctx.handle, *a, _ptr(app.mSpotLights), n, C.byref(sd), _stream(ctx.device)))
        elif entry == "point_shadows":
            built_lib.check(lib.crychic_draw_hot_path_point_shadows(ctx.handle, *a, _ptr(app.mSpotLights), n, C.byref(sd), None,
                                                                    _stream(ctx.device)))
        elif entry == "shared_spots_shadowed":
            built_lib.check(lib.crychic_draw_hot_path_shared_spots_shadowed(ex.handle, *a, None, 2, _ptr(app.mSpotLights), n, C.byref(sd),
                                                                            _stream(ctx.device)))
        else:
            d0 = _point_desc(None)
            built_lib.check(lib.crychic_draw_hot_path_shared_point_shadows(ex.handle, *a, None, 2, _ptr(app.mSpotLights), n, C.byref(sd),
                                                                           C.byref(d0), _stream(ctx.device)))
        torch.cuda.synchronize()
        frames.append(app.mBackBuffer.cpu().numpy().copy())
    for k in range(1, 4):
        assert np.array_equal(frames[0], frames[k]), k
    ex.close()
    ctx.close()


@pytest.mark.gpu
def test_point_shadow_argument_errors(built_lib):
    """count > 4, count > numPointLights, a NULL map among the first count and dim outside 16 .. 16384 are CRYCHIC_E_INVALID_ARG with
    a message on every new entry, and the output is left untouched."""
    import torch
    from crychic_renderer_amd import Context, sharding
    from crychic_renderer_amd.renderer import _ptr, _stream
    W, H = 64, 48
    lib = built_lib.lib
    ctx = Context(0)
    pl, p, dev = _device_scene(ctx, W, H)
    c = pl["consts"]
    points = shadowed_points()
    dp = _dev_lights(ctx, points)
    cubes = torch.zeros((4, 6, 16, 16), dtype=torch.int32, device=ctx.device)
    projs = [CENTRE_P] * 4
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
    app = _app(ctx, W, H, dev, c)
    app.set_point_lights(points)
    app.mBackBuffer.zero_()
    ex = sharding.StripExchange(ctx, W, H, 1, 0, sharding.StripExchange.new_unique_id(), slots=1)
    bad = []
    d = _point_desc(cubes, projs); d.count = 5; bad.append((d, dp))
    d = _point_desc(cubes, projs, count=3); bad.append((d, (dp[0], 2)))
    d = _point_desc(cubes, projs, count=3); d.maps[1] = None; bad.append((d, dp))
    for dim in (0, 15, 16385):
        d = _point_desc(cubes, projs, count=2); d.dim = dim; bad.append((d, dp))
    for d, (pd, pn) in bad:
        rc, _, _ = _light(lib, ctx, c.pass_cb, dev, W, H, 0, (pd, pn), (None, 0), None, d, out=out, rad=None)
        assert rc == -1 and b"point shadows" in lib.crychic_last_error()
        f = app.frame_desc()
        f.numPointLights = pn
        a = (C.byref(app.mSsaoCB), C.byref(app.mMainPassCB), C.byref(f))
        rc = lib.crychic_draw_hot_path_point_shadows(ctx.handle, *a, None, 0, None, C.byref(d), _stream(ctx.device))
        assert rc == -1 and b"point shadows" in lib.crychic_last_error()
        rc = lib.crychic_draw_hot_path_shared_point_shadows(ex.handle, *a, None, 1, None, 0, None, C.byref(d), _stream(ctx.device))
        assert rc == -1 and b"point shadows" in lib.crychic_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not app.mBackBuffer.any()
    ex.close()
    ctx.close()


@pytest.mark.gpu
def test_six_face_producer_matches_or_raster(built_lib, oracle):
    """The six faces of two shadowed point lights (12 targets, one crychic_draw_scene_to_shadow_maps call) render the reference scene
    bit-identically to oracle/or_raster.c."""
    import torch
    from crychic_renderer_amd import Context, geometry as g
    ctx = Context(0)
    sitems = g.cascade_scene_items(shadow_layer=True)
    lights = shadowed_points()
    dim = 128
    cubes, _ = _produce_cubes(ctx, lights, 2, dim)
    torch.cuda.synchronize()
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    seen = 0
    for k, (views, lp, _) in enumerate(point_transforms(lights, 2, dim)):
        for f in range(6):
            ref = oracle_lib.rasterize(oracle, 0, eye, (views[f] @ lp).astype(np.float32).T.reshape(-1), sitems, None, None, dim, dim,
                                       10000, 2.0)["depth"]
            assert np.array_equal(cubes[k, f].cpu().numpy().view(np.uint32), ref), (k, f)
            seen += (ref < 0xFFFFFF).any()
    assert seen >= 8
    ctx.close()


@pytest.mark.gpu
def test_reference_scene_point_shadows_end_to_end(built_lib, oracle):
    """The reference scene with four point lights above boxes, everything produced on the device and the faces rendered by
    Crychic.set_point_shadows(4, geometry=...): the frame equals the checker fed the device's planes and faces; a shadow never adds
    light, and ground pixels in the boxes' shadows get darker."""
    import torch
    from crychic_renderer_amd import Context, Crychic, LIGHT_SKY, SceneGeometry, geometry as g, scene
    import raster_util
    W, H, SD = 320, 240, 512
    ctx = Context(0)
    consts = raster_util.frame_constants(W, H, SD)
    items, sitems = g.cascade_scene_items(), g.cascade_scene_items(shadow_layer=True)
    geo = SceneGeometry(ctx, items, g.reference_materials(), g.procedural_textures(64))
    sgeo = SceneGeometry(ctx, sitems)
    cube = scene.make_cubemap(32, ctx.device)
    app = Crychic(ctx, W, H, torch.from_numpy(consts.randvec.copy()).to(ctx.device), cube, shadow_dim=SD)
    app.mMainPassCB, app.mSsaoCB = consts.pass_cb, consts.ssao_cb
    cbs = []
    for k in range(4):
        cb = built_lib.PassConstants(); cb.ViewProj[:] = list(raster_util.light_viewproj_t(consts, k)); cbs.append(cb)
    sgeo.DrawSceneToShadowMaps(cbs, [app.mShadowMap.mShadowMap[k] for k in range(4)])
    geo.DrawNormalsDepthAndGBuffer(app.mMainPassCB, app.mSsao.mNormalMap, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    app.blurCount, app.numDirLights, app.flags = 3, 1, LIGHT_SKY
    lights = scene.shadow_point_lights(4)
    app.set_point_lights(lights)
    app.set_point_shadows(4, dim=512, geometry=sgeo)
    app.Draw()
    torch.cuda.synchronize()
    got = app.mBackBuffer.cpu().numpy().copy()
    cubes = app.mPointShadowMaps.cpu().numpy().view(np.uint32)
    p = {"g0": app.mDeferred.mGBuffer[0].cpu().numpy(), "g1": app.mDeferred.mGBuffer[1].cpu().numpy(),
         "g2": app.mDeferred.mGBuffer[2].cpu().numpy(), "depth": app.mDepthStencilBuffer.cpu().numpy().view(np.uint32),
         "shadow": np.stack([app.mShadowMap.mShadowMap[k].cpu().numpy().view(np.uint32) for k in range(4)]),
         "cube": cube.cpu().numpy()}
    ao = app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16)
    pcb = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
    projs = [sp.reshape(-1) for _, _, sp in point_transforms(lights, 4, 512)]
    ps = point_shadow_lib.load()
    ref, lit1 = ps.checker(pcb, p, ao, 1, app.pcfSearchRadius, 1, points=lights, cubes=cubes, projs=projs)
    assert np.array_equal(got, ref)
    _, lit0 = ps.checker(pcb, p, ao, 1, app.pcfSearchRadius, 1, points=lights)
    assert (lit1[..., :3] <= lit0[..., :3]).all()
    darker = (lit1[..., :3] < lit0[..., :3]).all(-1)
    ground = (np.abs(p["g0"][..., 1]) < 1e-3) & ((p["depth"] & 0xFFFFFF) < 0xFFFFFF)
    assert (darker & ground).sum() > 50, int((darker & ground).sum())
    ctx.close()
