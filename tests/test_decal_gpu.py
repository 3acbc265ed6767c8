"""crychic_apply_decals on the device: the kernel against the checker (tests/decal_ref) byte for byte on the corpus of the CPU tier,
on planes behind guard bytes and 0, 16 and 32 bytes past a 64-byte boundary, in row ranges; known answers against numpy; and the pass
in front of Crychic.Draw -- against the lighting oracle fed the checker's planes, replayed from a graph, and per strip."""
import ctypes as C

import numpy as np
import pytest

import decal_lib as dl
from post_pass_lib import DevicePlanes, dev      # noqa: F401 -- dev: the module's fixture

pytestmark = pytest.mark.gpu


def run_device(dev, frame, mix, decals, textures, ranges=None, misalign=0, planes=None):
    """crychic_apply_decals over each (row0, rows) of `ranges` (default: the whole frame) on guarded device copies of the frame's
    planes in the formats of `mix`; returns the three planes as numpy bytes, the guards, the depth plane, the decals and the textures
    checked."""
    lib, ctx, torch = dev
    H, W = frame.H, frame.W
    host = frame.planes(mix) if planes is None else planes
    planes = DevicePlanes(dev)
    g = [planes.upload("G%d" % k, p, misalign, writable=True) for k, p in enumerate(host)]
    depth = planes.upload("depth", frame.depth, misalign)
    decals = np.ascontiguousarray(decals)
    dec = planes.upload("decals", decals, 0) if len(decals) else None
    tex = [planes.upload("texture %d" % k, t[0], 0) for k, t in enumerate(textures)]
    table = (lib.Texture * max(len(textures), 1))()
    for k, t in enumerate(textures):
        table[k] = lib.Texture(tex[k].data_ptr(), t[1], t[2], t[3])
    pcb = frame.pass_constants()
    s = torch.cuda.current_stream(ctx.device)
    for row0, rows in (ranges or [(0, H)]):
        lib.check(lib.lib.crychic_apply_decals(ctx.handle, C.byref(pcb), C.c_void_p(depth.data_ptr()), C.c_void_p(g[0].data_ptr()),
                                               C.c_void_p(g[1].data_ptr()), C.c_void_p(g[2].data_ptr()), dl.MIXES[mix],
                                               None if dec is None else C.c_void_p(dec.data_ptr()), len(decals), table, len(textures), W, H, row0,
                                               rows, C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return [v.cpu().numpy().reshape(p.shape) for v, p in zip(g, host)]


def assert_planes_equal(got, want, name):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "%s: G%d differs from the checker in %d bytes" % (name, k, int((a != b).sum()))


@pytest.mark.parametrize("name", dl.case_names())
def test_device_equals_checker(dev, name):
    k = dl.case_names().index(name)
    _, frame, decals, textures, mix = dl.case(name)
    got = run_device(dev, frame, mix, decals, textures, misalign=(0, 16, 32)[k % 3])
    assert_planes_equal(got, dl.expected(name)[0], name)


@pytest.mark.parametrize("name", ["scene_all_f32", "scene_all_mixed", "scene_all_f16", "130x9_n64_f16", "65x7_n64_mixed"])
def test_row_ranges_stitch_to_the_whole_frame(dev, name):
    _, frame, decals, textures, mix = dl.case(name)
    H = frame.H
    cuts = sorted({0, 1, H // 3, H // 3 + 1, (2 * H) // 3 | 1, H})
    ranges = [(a, b - a) for a, b in zip(cuts, cuts[1:]) if b <= H] + [(H, 0)]
    ranges = [r for r in ranges if r[0] + r[1] <= H]
    got = run_device(dev, frame, mix, decals, textures, ranges=ranges)
    assert_planes_equal(got, dl.expected(name)[0], name)
    # one range alone leaves every other row as it was
    r0, rn = cuts[1], cuts[2] - cuts[1]
    part = run_device(dev, frame, mix, decals, textures, ranges=[(r0, rn)])
    want = dl.checker(frame, mix, decals, textures, r0, rn)[0]
    assert_planes_equal(part, want, name + " rows")
    for p, q in zip(part, frame.planes(mix)):
        assert np.array_equal(p[:r0], q[:r0]) and np.array_equal(p[r0 + rn:], q[r0 + rn:])


def test_no_decals_and_a_decal_in_the_air_change_nothing(dev):
    sc = dl.scene_frame()
    tex = [dl.solid_texture((255, 255, 255, 255))]
    air = dl.decal_from_box(dl.floor_world((0.0, 30.0, 0.0), (3.0, 1.0, 3.0)), (1, 1), flags=15)
    for decals in (dl.decals_array([]), air):
        got = run_device(dev, sc, "f32", decals, tex)
        assert_planes_equal(got, sc.planes("f32"), "unchanged")


def test_opaque_texel_known_answer(dev):
    """A 1 x 1 opaque texel, opacity 1, no fade: the albedo inside the box is (tint - x) + x, every other byte as it was."""
    sc = dl.scene_frame()
    tint = np.array([0.9, 0.5, 0.2], np.float32)
    rec = dl.decal_from_box(dl.floor_world((2.5, 0.0, -7.5), (1.5, 0.25, 1.5)), (1, 1), tint=tint)
    got = run_device(dev, sc, "f32", rec, [dl.solid_texture((255, 255, 255, 255))])
    P = sc.g[0][..., :3].astype(np.float64)
    q = np.stack([np.abs(P @ rec["invWorld"][0][4 * c:4 * c + 3].astype(np.float64) + rec["invWorld"][0][4 * c + 3]) for c in range(3)], -1)
    covered = (sc.depth & 0xFFFFFF) < 0xFFFFFF
    inside = covered & (q < 0.4999).all(-1)          # clear of the faces, where float32 and float64 could disagree
    assert inside.sum() > 400
    x = sc.g[1][..., :3]
    want = (tint[None, None, :] - x) + x
    g1 = got[1].view(np.float32)
    assert np.array_equal(g1[inside][:, :3], want[inside])
    outside = ~(covered & (q < 0.5001).all(-1))
    assert np.array_equal(g1[outside], sc.g[1][outside]) and np.array_equal(g1[..., 3], sc.g[1][..., 3])
    assert np.array_equal(got[0], sc.planes("f32")[0]) and np.array_equal(got[2], sc.planes("f32")[2])


def test_order_matters_and_a_decal_facing_away_does_nothing(dev):
    sc = dl.scene_frame()
    tex = [dl.solid_texture((255, 255, 255, 200))]
    a = dl.decal_from_box(dl.floor_world((2.5, 0.0, -7.5), (1.5, 0.25, 1.5)), (1, 1), tint=(1.0, 0.0, 0.0))
    b = dl.decal_from_box(dl.floor_world((3.0, 0.0, -7.0), (1.5, 0.25, 1.5)), (1, 1), tint=(0.0, 0.0, 1.0))
    ab, ba = dl.decals_array([a, b]), dl.decals_array([b, a])
    got_ab, got_ba = run_device(dev, sc, "f32", ab, tex), run_device(dev, sc, "f32", ba, tex)
    assert not np.array_equal(got_ab[1], got_ba[1])
    assert_planes_equal(got_ab, dl.checker(sc, "f32", ab, tex)[0], "a then b")
    assert_planes_equal(got_ba, dl.checker(sc, "f32", ba, tex)[0], "b then a")
    # the same box looking up from below the floor: its normalW points down, the fade is 0 everywhere
    down = dl.box_world((2.5, 0.0, -7.5), (1.5, 1.5, 0.25), rot=np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]))
    away = dl.decal_from_box(down, (1, 1), 0.5, 0.0, flags=15)
    assert_planes_equal(run_device(dev, sc, "f32", away, tex), sc.planes("f32"), "facing away")


def test_level_rises_with_view_depth_and_addressing_clamps(dev):
    """The two texture known answers against numpy, on the device: det_log2's level choice with the trilinear blend, and CLAMP."""
    frame, rec, tex = dl.grey_levels_case()
    dl.assert_grey_does_not_fall(frame, rec, run_device(dev, frame, "f32", rec, tex)[1])
    frame, rec, tex = dl.red_blue_case()
    dl.assert_red_blue(run_device(dev, frame, "f32", rec, tex)[1])


# ---- behind Crychic ----------------------------------------------------------------------------------------------------------------

def scene_decals():
    from crychic_renderer_amd import geometry as g, DECAL_ALBEDO, DECAL_ROUGHNESS, DECAL_NORMAL, DECAL_METALNESS
    textures = [g.decal_texture("disc", 16), g.decal_texture("dent", 16), g.decal_texture("ring", 8)]
    decals = [g.decal_from_box(g.decal_box_world((2.5, 0.0, -7.5), (1.5, 0.25, 1.5)), (16, 16), 0.5, 0.0, texture=0, normalTexture=1,
                               flags=DECAL_ALBEDO | DECAL_ROUGHNESS | DECAL_NORMAL, roughness=0.05),
              g.decal_from_box(g.decal_box_world((0.0, 0.8, -10.8), (0.6, 0.6, 0.3), down=False), (8, 8), 0.5, 0.0, texture=2,
                               flags=DECAL_ALBEDO | DECAL_METALNESS, metalness=0.8, tint=(0.9, 0.1, 0.1))]
    return decals, textures


def lit_reference(planes, app, g_planes, mix):
    """The lighting oracle's frame for the scene's inputs with the G-buffer planes `g_planes` (bytes in the formats of `mix`)."""
    import oracle_lib
    import scene_util
    orc = oracle_lib.load()
    p = scene_util.np_planes(planes)
    c = planes["consts"]
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    ao = orc.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)
    g = [np.ascontiguousarray(b.view(np.float16).astype(np.float32) if b.shape[2] == 8 else b.view(np.float32)) for b in g_planes]
    return orc.deferred_light(pcb, g[0], g[1], g[2], p["depth"], ao, p["shadow"], p["cube"], 3, app.pcfSearchRadius, sky=True)


@pytest.fixture(scope="module")
def scene_apps(dev):
    lib, ctx, torch = dev
    from crychic_renderer_amd import Crychic, LIGHT_SKY, scene
    W, H, SD = 128, 96, 256
    planes = scene.make_scene(W, H, shadow_dim=SD, cube_dim=32, device="cuda:0")
    apps = {}
    for mix in dl.MIXES:
        app = Crychic(ctx, W, H, planes["randvec"], planes["cube"], shadow_dim=SD, gbuffer_formats=mix)
        app.load_scene(planes)
        app.blurCount, app.numDirLights, app.flags = 3, 3, LIGHT_SKY
        apps[mix] = app
    return planes, apps


def host_decals(decals, textures):
    recs = dl.decals_array([np.frombuffer(bytes(d), dl.DECAL).copy() for d in decals])
    return recs, [(np.ascontiguousarray(t[0], np.uint8), t[1], t[2], t[3]) for t in textures]


@pytest.mark.parametrize("mix", list(dl.MIXES))
def test_apply_decals_then_draw_equals_the_oracle_on_the_checkers_planes(dev, scene_apps, mix):
    lib, ctx, torch = dev
    planes, apps = scene_apps
    app = apps[mix]
    pristine = [g.clone() for g in app.mDeferred.mGBuffer]
    decals, textures = scene_decals()
    recs, tex = host_decals(decals, textures)
    f = np.frombuffer(bytes(planes["consts"].pass_cb), np.float32)
    frame = dl.Frame(f[0:16], f[32:48], planes["depth"].cpu().numpy().view(np.uint32), *[planes["g%d" % k].cpu().numpy() for k in range(3)])
    want_planes, n = dl.checker(frame, mix, recs, tex)
    assert n["store_albedo"] > 500 and n["store_normal"] > 200 and n["store_metalness"] > 500
    try:
        app.set_decals(decals, textures)
        app.apply_decals()
        app.Draw()
        torch.cuda.synchronize()
        got_planes = [g.cpu().numpy().view(np.uint8).reshape(w.shape) for g, w in zip(app.mDeferred.mGBuffer, want_planes)]
        assert_planes_equal(got_planes, want_planes, mix)
        want = lit_reference(planes, app, want_planes, mix)
        got = app.mBackBuffer.cpu().numpy()
        assert np.array_equal(got, want), "frame differs from the oracle in %d bytes" % int((got != want).sum())
        plain = lit_reference(planes, app, [p.cpu().numpy().view(np.uint8).reshape(w.shape) for p, w in zip(pristine, want_planes)], mix)
        assert int((want != plain).any(-1).sum()) > 500, "the decals do not show in the lit frame"
        if mix == "f32":
            # a graph of [restore the pristine planes, decals, Draw] replays to the same frame; a strip equals the frame's rows
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for g, p in zip(app.mDeferred.mGBuffer, pristine):
                    g.copy_(p)
                app.apply_decals()
                app.Draw()
            for _ in range(2):
                app.mBackBuffer.zero_()
                torch.cuda.synchronize()
                graph.replay()
                torch.cuda.synchronize()
                assert np.array_equal(app.mBackBuffer.cpu().numpy(), want)
            for g, p in zip(app.mDeferred.mGBuffer, pristine):
                g.copy_(p)
            app.mBackBuffer.zero_()
            app.apply_decals(row0=32, rows=32)
            app.Draw(row0=32, rows=32)
            torch.cuda.synchronize()
            assert np.array_equal(app.mBackBuffer.cpu().numpy()[32:64], want[32:64])
    finally:
        app.set_decals([])
        for g, p in zip(app.mDeferred.mGBuffer, pristine):
            g.copy_(p)
