"""The C entries of one pass family against each other, called directly (the Python methods reach only the widest of them): every
narrower entry writes the bytes the widest one writes with NULL / 0 in the arguments it does not take, and a refused call keeps its
status and its message."""
import ctypes as C

import numpy as np
import pytest

import raster_util
from local_lights_util import _dev_lights, _device_scene, points_for_test, random_maps, spot_transforms, spots_for_test, transposed, with_transforms

torch = pytest.importorskip("torch")

# two 64-pixel columns and a remainder, a partial last workgroup row; 64 x 64 cascades, an 8-texel cube map
W, H, SD, CD = 130, 22, 64, 8
POISON32, POISON16 = 0x7FC01234, 0x7E12


@pytest.fixture(scope="module")
def ctx(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


def _bytes_equal(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


# ---- producers ------------------------------------------------------------------------------------------------------------------

class _Producers:
    """The reference scene's camera and shadow geometry on the device, and the producer entries by name."""

    def __init__(self, ctx, lib):
        from crychic_renderer_amd import SceneGeometry, geometry as g
        from crychic_renderer_amd.renderer import _ptr, _stream
        self.ctx, self.lib, self._ptr = ctx, lib, _ptr
        self.consts = raster_util.frame_constants(W, H, SD)
        self.geo = SceneGeometry(ctx, g.cascade_scene_items(), g.reference_materials(), g.procedural_textures(64))
        self.sgeo = SceneGeometry(ctx, g.cascade_scene_items(shadow_layer=True))
        self.stream = _stream(ctx.device)

    def planes(self):
        """(normal, g0, g1, g2, depth), every texel a poison word."""
        dev = self.ctx.device
        n = torch.full((H, W, 4), POISON16, dtype=torch.int16, device=dev).view(torch.float16)
        g = [torch.full((H, W, 4), POISON32, dtype=torch.int32, device=dev).view(torch.float32) for _ in range(3)]
        return [n] + g + [torch.full((H, W), POISON32, dtype=torch.int32, device=dev)]

    def camera(self, entry, normal, rows=None, formats=False, cb=True, g0=True, textures=True, target=(W, H)):
        """One call of the G-buffer entry `entry` on fresh planes; normal: the entry takes a normal map.  rows: the (gRow0, gRows) the
        _rows entries take; formats: the (flags, gRow0, gRows) of the _formats entry.  Returns (status, planes)."""
        p, geo, ptr = self.planes(), self.geo, self._ptr
        ws = geo.workspace(W, H)
        a = [self.ctx.handle, C.byref(self.consts.pass_cb) if cb else None, geo.items, len(geo.items), ptr(geo.materials), geo.n_materials,
             geo.textures if textures else None, geo.n_textures]
        if formats is not False:
            a += [ptr(p[0]) if normal else None, ptr(p[1]) if g0 else None, ptr(p[2]), ptr(p[3]), formats[0], ptr(p[4]), *target, formats[1], formats[2]]
        else:
            a += ([ptr(p[0])] if normal else []) + [ptr(p[1]) if g0 else None, ptr(p[2]), ptr(p[3]), ptr(p[4]), *target] + list(rows or ())
        rc = getattr(self.lib, entry)(*a, ptr(ws), ws.numel(), self.stream)
        torch.cuda.synchronize()
        return rc, (p if normal else p[1:])


@pytest.fixture(scope="module")
def producers(ctx, built_lib):
    return _Producers(ctx, built_lib.lib)


@pytest.mark.gpu
@pytest.mark.parametrize("normal,plain,rows", [(False, "crychic_draw_gbuffer", "crychic_draw_gbuffer_rows"),
                                               (True, "crychic_draw_normals_depth_and_gbuffer", "crychic_draw_normals_depth_and_gbuffer_rows")])
def test_gbuffer_entries_write_the_same_bytes(producers, normal, plain, rows):
    """entry == _rows(0, H) == _formats(flags 0, 0, 0) on the whole target; on one strip _rows == _formats, poison outside it."""
    rc, whole = producers.camera(plain, normal)
    assert rc == 0
    depth = whole[-1]
    assert bool((depth < 0xFFFFFF).any())                                               # the scene is in view
    for g in whole[:-1]:
        assert not bool((g.view(torch.int32 if g.dtype == torch.float32 else torch.int16) == (POISON32 if g.dtype == torch.float32 else POISON16)).all())
    rc, a = producers.camera(rows, normal, rows=(0, H))
    assert rc == 0 and _bytes_equal(a, whole)
    rc, b = producers.camera("crychic_draw_gbuffer_formats", normal, formats=(0, 0, 0))
    assert rc == 0 and _bytes_equal(b, whole)
    r0, rn = 5, 9
    rc, a = producers.camera(rows, normal, rows=(r0, rn))
    assert rc == 0
    rc, b = producers.camera("crychic_draw_gbuffer_formats", normal, formats=(0, r0, rn))
    assert rc == 0 and _bytes_equal(a, b)
    outside = torch.ones(H, dtype=torch.bool, device=depth.device)
    outside[r0:r0 + rn] = False
    for t, full in zip(a[-4:-1], whole[-4:-1]):                                         # G0..G2
        assert torch.equal(t[r0:r0 + rn].view(torch.int32), full[r0:r0 + rn].view(torch.int32))
        assert bool((t[outside].view(torch.int32) == POISON32).all())


@pytest.mark.gpu
def test_four_shadow_passes_equal_the_fused_pass(producers, built_lib):
    """crychic_draw_scene_to_shadow_map once per cascade == crychic_draw_scene_to_shadow_maps with the four of them."""
    lib, sgeo, ptr, dev = producers.lib, producers.sgeo, producers._ptr, producers.ctx.device
    cbs = (built_lib.PassConstants * 4)()
    for k in range(4):
        cbs[k].ViewProj[:] = list(raster_util.light_viewproj_t(producers.consts, k))
    single = torch.full((4, SD, SD), POISON32, dtype=torch.int32, device=dev)
    fused = torch.full((4, SD, SD), POISON32, dtype=torch.int32, device=dev)
    ws = sgeo.workspace(SD, SD, 4)
    for k in range(4):
        built_lib.check(lib.crychic_draw_scene_to_shadow_map(producers.ctx.handle, C.byref(cbs[k]), sgeo.items, len(sgeo.items), ptr(single[k]), SD,
                                                             10000, 2.0, ptr(ws), ws.numel(), producers.stream))
    targets = (C.c_void_p * 4)(*[fused[k].data_ptr() for k in range(4)])
    built_lib.check(lib.crychic_draw_scene_to_shadow_maps(producers.ctx.handle, C.cast(cbs, C.c_void_p), 4, sgeo.items, len(sgeo.items),
                                                          C.cast(targets, C.c_void_p), SD, 10000, 2.0, ptr(ws), ws.numel(), producers.stream))
    torch.cuda.synchronize()
    assert torch.equal(single, fused)
    assert bool((single < 0xFFFFFF).any()) and not bool((single == POISON32).any())


# ---- lighting and the hot path --------------------------------------------------------------------------------------------------

class _Lit:
    """scene_util.cpu_scene at W x H (the fixture accepts this size) on the device with two point and two spot lights, the first spot
    light shadowed by one 16 x 16 map."""

    def __init__(self, ctx, lib):
        from crychic_renderer_amd._lib import Light, SpotShadows
        from crychic_renderer_amd.renderer import _ptr, _stream
        self.ctx, self.lib, self._ptr, self.stream = ctx, lib, _ptr, _stream(ctx.device)
        self.pl, _, self.dev = _device_scene(ctx, W, H, SD, CD)
        points, spots = (Light * 2)(*points_for_test()[:2]), (Light * 2)(*spots_for_test()[:2])
        self.points, self.spots = _dev_lights(ctx, points), _dev_lights(ctx, spots)
        self.maps = torch.from_numpy(random_maps(1, 16, 7).view(np.int32)).to(ctx.device)
        self.sdesc = SpotShadows()
        self.sdesc.count, self.sdesc.dim = 1, 16
        self.sdesc.maps[0] = self.maps[0].data_ptr()
        self.cb = with_transforms(self.pl["consts"].pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 1)])[0]
        self.sh = (C.c_void_p * 4)(*[self.dev["shadow"][k].data_ptr() for k in range(4)])

    def light(self, entry, tail, flags=1, rows=(0, H), size=(W, H), cube_dim=CD):
        """crychic_deferred_light<entry> with `tail` behind the flags; returns (status, out, radiance)."""
        dev, ptr = self.dev, self._ptr
        out = torch.full((H, W, 4), 7, dtype=torch.uint8, device=self.ctx.device)
        rad = torch.full((H, W, 4), 7.0, dtype=torch.float32, device=self.ctx.device)
        rc = getattr(self.lib, "crychic_deferred_light" + entry)(
            self.ctx.handle, C.byref(self.cb), ptr(dev["g0"]), ptr(dev["g1"]), ptr(dev["g2"]), ptr(dev["depth"]), None, self.sh, SD, ptr(dev["cube"]),
            cube_dim, ptr(out), ptr(rad), *size, *rows, 3, 0.0, flags, *tail, self.stream)
        torch.cuda.synchronize()
        return rc, out, rad


@pytest.fixture(scope="module")
def lit(ctx, built_lib):
    return _Lit(ctx, built_lib.lib)


@pytest.mark.gpu
def test_deferred_light_entries_write_the_same_bytes(lit):
    """Each narrower crychic_deferred_light* entry == crychic_deferred_light_point_shadows with the lists it does not take NULL / 0.
    (test_spot_lights.py has _points == _spots with no spot lights, test_point_shadows.py the descriptors with count 0; here the
    lists are there and the narrower entry leaves the later ones out.)"""
    p, s, sd = (lit._ptr(lit.points[0]), lit.points[1]), (lit._ptr(lit.spots[0]), lit.spots[1]), C.byref(lit.sdesc)
    none = (None, 0)
    frames = []
    for entry, own, wide in (("", (), (*none, *none, None, None)), ("_points", p, (*p, *none, None, None)),
                             ("_spots", (*p, *s), (*p, *s, None, None)), ("_spots_shadowed", (*p, *s, sd), (*p, *s, sd, None))):
        rc, out, rad = lit.light(entry, own)
        rc2, out2, rad2 = lit.light("_point_shadows", wide)
        assert rc == 0 and rc2 == 0, entry
        assert torch.equal(out, out2) and torch.equal(rad.view(torch.int32), rad2.view(torch.int32)), entry
        frames.append(out)
    for k in range(1, 4):         # every list changes the frame: no entry is compared on arguments it ignores
        assert not torch.equal(frames[k - 1], frames[k]), k


@pytest.mark.gpu
def test_hot_path_entries_write_the_same_bytes(lit, built_lib):
    """crychic_draw_hot_path, _spots and _spots_shadowed == crychic_draw_hot_path_point_shadows with the arguments they do not take
    NULL / 0: blurCount 2, the point lights in the frame descriptor.  (test_spot_lights.py has crychic_draw_hot_path == _spots and
    the _shared pair with no spot lights, test_point_shadows.py _spots_shadowed == _point_shadows and the _shared pair with a NULL
    point descriptor on its own frame; they are not repeated for the _shared entries.)"""
    from crychic_renderer_amd import Crychic, LIGHT_SKY
    from crychic_renderer_amd._lib import Light
    ctx, lib = lit.ctx, lit.lib
    app = Crychic(ctx, W, H, lit.dev["randvec"], lit.dev["cube"], shadow_dim=SD)
    app.load_scene({**lit.dev, "consts": lit.pl["consts"]})
    app.blurCount, app.numDirLights, app.flags = 2, 3, LIGHT_SKY
    app.set_point_lights((Light * 2)(*points_for_test()[:2]))
    f = app.frame_desc()
    head = (ctx.handle, C.byref(app.mSsaoCB), C.byref(lit.cb), C.byref(f))
    s, sd = (lit._ptr(lit.spots[0]), lit.spots[1]), C.byref(lit.sdesc)

    def frame(entry, tail):
        app.mBackBuffer.fill_(3)
        app.mSsao.mAmbientMap0.fill_(5)
        built_lib.check(getattr(lib, "crychic_draw_hot_path" + entry)(*head, *tail, lit.stream))
        torch.cuda.synchronize()
        return app.mBackBuffer.clone(), app.mSsao.mAmbientMap0.clone()

    frames = []
    for entry, own, wide in (("", (), (None, 0, None, None)), ("_spots", s, (*s, None, None)), ("_spots_shadowed", (*s, sd), (*s, sd, None))):
        a, b = frame(entry, own), frame("_point_shadows", wide)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), entry
        frames.append(a[0])
    assert not torch.equal(frames[0], frames[1]) and not torch.equal(frames[1], frames[2])
    assert not bool((frames[0] == 3).all()) and not bool((a[1] == 5).all())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

# The messages are the parent commit's literals (api.cpp before the checks were merged), written out: not read from the library.
G_NULL, F_NULL, T_NULL = b"null G-buffer target", b"null normal / G-buffer target", b"null texture table"
G_ROWS = b"G-buffer rows [%d,+%d) outside the 22-row target"
CAMERA = ["crychic_draw_gbuffer", "crychic_draw_normals_depth_and_gbuffer", "crychic_draw_gbuffer_rows", "crychic_draw_normals_depth_and_gbuffer_rows",
          "crychic_draw_gbuffer_formats", "crychic_draw_gbuffer_formats"]


def _camera_kwargs(k, r0=0, rn=H):
    """The camera() arguments of CAMERA[k] (the _formats entry twice: without and with a normal map) for rows [r0, r0 + rn)."""
    normal = bool(k & 1)
    if k >= 4:
        return dict(normal=normal, formats=(0, r0, rn))
    return dict(normal=normal, rows=(r0, rn) if k >= 2 else None)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(6))
def test_camera_entry_refusals(producers, k):
    """Every G-buffer entry: a null target, a null texture table, rows outside the target; gRows == 0 on the _rows entries only."""
    lib, entry = producers.lib, CAMERA[k]
    fused = k in (1, 3)             # the entries with a normal map of their own name it in the message
    cases = [(dict(g0=False), F_NULL if fused else G_NULL), (dict(textures=False), T_NULL)]
    if k >= 2:
        cases += [(_camera_kwargs(k, 20, 3), G_ROWS % (20, 3)), (_camera_kwargs(k, 23, 0), G_ROWS % (23, 0))]
    if k in (2, 3):
        cases += [(_camera_kwargs(k, 4, 0), G_ROWS % (4, 0))]
    if k in (1, 3):
        cases += [(dict(normal=None), F_NULL)]
    if k >= 4:
        cases += [(dict(formats=(0x8000, 0, 0)), b"gbufferFlags 0x8000: bits outside CRYCHIC_GBUFFER_G0_F16 | G1_F16 | G2_F16")]
    # shared by every entry, behind its own checks (raster_common): the pass constants, the target's size
    cases += [(dict(cb=False), b"null argument"), (dict(target=(1 << 20, 2)), b"target 1048576x2 exceeds 2^28 pixels, 2^20 columns or 262140 rows")]
    for extra, message in cases:
        kw = _camera_kwargs(k)
        if "target" in extra and k >= 2:                # rows inside the 2-row target, so that its size is what is refused
            kw = _camera_kwargs(k, 0, 2)
        if extra.get("normal", 0) is None:              # a fused entry without its normal map: pass NULL in its place
            rc = _fused_null_normal(producers, entry, k)
        else:
            kw.update(extra)
            rc, planes = producers.camera(entry, **kw)
            for t in planes:                            # nothing was launched
                assert bool((t.view(torch.int16 if t.dtype == torch.float16 else torch.int32) == (POISON16 if t.dtype == torch.float16 else POISON32)).all())
        assert rc == (-4 if b"exceeds" in message else -1), (entry, extra)
        assert lib.crychic_last_error() == message, (entry, extra)
    if k >= 4:          # _formats reads gRows == 0 as the whole target
        rc, _ = producers.camera(entry, **_camera_kwargs(k, 4, 0))
        assert rc == 0


def _fused_null_normal(producers, entry, k):
    p, geo, ptr = producers.planes(), producers.geo, producers._ptr
    ws = geo.workspace(W, H)
    a = [producers.ctx.handle, C.byref(producers.consts.pass_cb), geo.items, len(geo.items), ptr(geo.materials), geo.n_materials, geo.textures,
         geo.n_textures, None, ptr(p[1]), ptr(p[2]), ptr(p[3]), ptr(p[4]), W, H] + ([0, H] if k == 3 else [])
    return getattr(producers.lib, entry)(*a, ptr(ws), ws.numel(), producers.stream)


@pytest.mark.gpu
def test_scene_geometry_refuses_an_explicit_strip_of_no_rows(producers):
    """SceneGeometry.DrawGBuffer / DrawNormalsDepthAndGBuffer(g_rows=(4, 0)): status -1, as the _rows entries answer."""
    from crychic_renderer_amd import CrychicError
    n, g0, g1, g2, d = producers.planes()
    for draw in (lambda: producers.geo.DrawGBuffer(producers.consts.pass_cb, [g0, g1, g2], d, g_rows=(4, 0)),
                 lambda: producers.geo.DrawNormalsDepthAndGBuffer(producers.consts.pass_cb, n, [g0, g1, g2], d, g_rows=(4, 0))):
        with pytest.raises(CrychicError) as e:
            draw()
        assert e.value.status == -1 and (G_ROWS % (4, 0)).decode() in str(e.value)
    torch.cuda.synchronize()
    assert bool((d == POISON32).all())


def _refusals(lit, built_lib):
    """(what, call, status, message): one wrong argument per use of the shared checks -- rows, frame bounds, cube levels, overlap,
    the environment lookups -- and per remaining producer entry."""
    lib, ctx, dev, ptr, st = lit.lib, lit.ctx, lit.dev, lit._ptr, lit.stream
    scb, pcb = lit.pl["consts"].ssao_cb, lit.cb
    h2 = torch.zeros((H // 2, W // 2), dtype=torch.int16, device=ctx.device)
    h2b = torch.zeros_like(h2)
    edge = torch.zeros((int(lib.crychic_edge_plane_bytes(W, H)),), dtype=torch.uint8, device=ctx.device)
    rgba, rgba2 = (torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device) for _ in range(2))
    chain = torch.zeros((4096,), dtype=torch.uint8, device=ctx.device)
    big = 1 << 20
    AMBIENT_ROWS = b"rows [%d,+%d) outside the 11-row ambient map"
    FRAME_ROWS = b"rows [%d,+%d) outside the 22-row frame"
    FRAME_BIG = b"frame 1048576x2 exceeds 2^28 pixels, 2^20 columns or 262140 rows"
    LEVELS = b"%d cube map levels, a 8-texel face has at most 4"
    DERIVATIVE = (b"CRYCHIC_LIGHT_AMBIENT_SH with a derivative-LOD chain: use no chain, or CRYCHIC_LIGHT_CUBE_LEVELS(n) with "
                  b"CRYCHIC_LIGHT_CUBE_GLOSS")
    n, d, r = ptr(dev["normal"]), ptr(dev["depth"]), ptr(dev["randvec"])
    sgeo_ws = torch.zeros((1 << 16,), dtype=torch.uint8, device=ctx.device)
    one = (built_lib.DrawItem * 1)()
    sm = torch.zeros((8, 8), dtype=torch.int32, device=ctx.device)
    cbs2 = (built_lib.PassConstants * 2)()
    maps2 = (C.c_void_p * 2)(sm.data_ptr(), None)

    def hot(flags=None, size=None):
        from crychic_renderer_amd import Crychic
        app = Crychic(ctx, W, H, dev["randvec"], dev["cube"], shadow_dim=SD)
        app.load_scene({**dev, "consts": lit.pl["consts"]})
        f = app.frame_desc()
        if flags is not None:
            f.flags = flags
        if size is not None:
            f.W, f.H, f.row0, f.rows = size[0], size[1], 0, size[1]
        return lib.crychic_draw_hot_path(ctx.handle, C.byref(scb), C.byref(pcb), C.byref(f), st)

    return [
        # rows
        ("ssao rows", lambda: lib.crychic_ssao(ctx.handle, C.byref(scb), n, d, r, ptr(h2), None, W, H, 12, 0, st), -1, AMBIENT_ROWS % (12, 0)),
        ("ssao_edges rows", lambda: lib.crychic_ssao_edges(ctx.handle, C.byref(scb), n, d, ptr(edge), W, H, 4, 8, st), -1, AMBIENT_ROWS % (4, 8)),
        ("ssao_blur rows", lambda: lib.crychic_ssao_blur(ctx.handle, C.byref(scb), ptr(edge), ptr(h2), ptr(h2b), W, H, 1, 0, 12, st), -1,
         AMBIENT_ROWS % (0, 12)),
        ("ssao_compute rows", lambda: lib.crychic_ssao_compute(ctx.handle, C.byref(scb), n, d, r, ptr(h2), ptr(h2b), ptr(edge), W, H, 2, 11, 1, st), -1,
         AMBIENT_ROWS % (11, 1)),
        ("deferred_light rows", lambda: lit.light("", (), rows=(20, 3))[0], -1, FRAME_ROWS % (20, 3)),
        ("antialias rows", lambda: lib.crychic_antialias(ctx.handle, ptr(rgba), ptr(rgba2), W, H, 23, 0, None, st), -1, FRAME_ROWS % (23, 0)),
        ("fog rows", lambda: lib.crychic_fog(ctx.handle, C.byref(pcb), d, lit.sh, SD, ptr(rgba), ptr(rgba), W, H, 0, 23, None, st), -1,
         FRAME_ROWS % (0, 23)),
        # frame bounds
        ("full-screen frame", lambda: lib.crychic_ssao(ctx.handle, C.byref(scb), n, d, r, ptr(h2), None, big, 2, 0, 1, st), -4, FRAME_BIG),
        ("deferred_light frame", lambda: lit.light("", (), size=(big, 2), rows=(0, 2))[0], -4, FRAME_BIG),
        ("hot path frame", lambda: hot(size=(big, 2)), -4, FRAME_BIG),
        ("antialias frame", lambda: lib.crychic_antialias(ctx.handle, ptr(rgba), ptr(rgba2), 1 << 15, 1 << 14, 0, 1, None, st), -4,
         b"frame 32768x16384 exceeds 2^28 pixels or 2097120 rows"),
        ("antialias frame rows", lambda: lib.crychic_antialias(ctx.handle, ptr(rgba), ptr(rgba2), 1, 2097121, 0, 1, None, st), -4,
         b"frame 1x2097121 exceeds 2^28 pixels or 2097120 rows"),
        ("fog frame", lambda: lib.crychic_fog(ctx.handle, C.byref(pcb), d, lit.sh, SD, ptr(rgba), ptr(rgba), 1 << 15, 1 << 14, 0, 1, None, st), -4,
         b"frame 32768x16384 exceeds 2^28 pixels"),
        ("shadow map target", lambda: lib.crychic_draw_scene_to_shadow_map(ctx.handle, C.byref(pcb), one, 0, ptr(sm), big, 0, 0.0, ptr(sgeo_ws),
                                                                          sgeo_ws.numel(), st), -4,
         b"target 1048576x1048576 exceeds 2^28 pixels, 2^20 columns or 262140 rows"),
        # the producers without a G-buffer
        ("shadow map null", lambda: lib.crychic_draw_scene_to_shadow_map(ctx.handle, C.byref(pcb), one, 0, None, 8, 0, 0.0, ptr(sgeo_ws), sgeo_ws.numel(), st),
         -1, b"null argument"),
        ("shadow maps null", lambda: lib.crychic_draw_scene_to_shadow_maps(ctx.handle, C.cast(cbs2, C.c_void_p), 2, one, 0, C.cast(maps2, C.c_void_p), 8, 0,
                                                                          0.0, ptr(sgeo_ws), sgeo_ws.numel(), st), -1, b"shadow target 1 is null"),
        ("normals null", lambda: lib.crychic_draw_normals_and_depth(ctx.handle, C.byref(pcb), one, 0, None, ptr(sm), 8, 8, ptr(sgeo_ws), sgeo_ws.numel(), st),
         -1, b"null normal target"),
        ("normals null depth", lambda: lib.crychic_draw_normals_and_depth(ctx.handle, C.byref(pcb), one, 0, ptr(h2), None, 8, 8, ptr(sgeo_ws),
                                                                         sgeo_ws.numel(), st), -1, b"null argument"),
        # cube levels
        ("deferred_light levels", lambda: lit.light("", (), flags=1 | (5 << 16))[0], -1, LEVELS % 5),
        ("hot path levels", lambda: hot(flags=1 | (5 << 16)), -1, LEVELS % 5),
        ("generate levels", lambda: lib.crychic_generate_cube_mips(ctx.handle, ptr(chain), 8, 0, st), -1, LEVELS % 0),
        ("prefilter levels", lambda: lib.crychic_prefilter_cube_chain(ctx.handle, ptr(chain), ptr(chain[2048:]), 8, 5, st), -1, LEVELS % 5),
        # overlap
        ("prefilter overlap", lambda: lib.crychic_prefilter_cube_chain(ctx.handle, ptr(chain), ptr(chain[4:]), 8, 1, st), -1,
         b"the source and destination chains overlap"),
        ("antialias overlap", lambda: lib.crychic_antialias(ctx.handle, ptr(rgba), ptr(rgba), W, H, 0, H, None, st), -1,
         b"the anti-aliasing input and output planes overlap (the pass cannot run in place)"),
        ("fog overlap", lambda: lib.crychic_fog(ctx.handle, C.byref(lit.pl["consts"].pass_cb), d, lit.sh, SD, ptr(rgba), ptr(rgba.view(-1)[4:]), W, H - 2,
                                                0, 1, None, st), -1, b"the fog input and output planes overlap (in place takes the same address)"),
        ("project overlap", lambda: lib.crychic_project_cube_sh(ctx.handle, ptr(chain), 8, ptr(chain[8:]), st), -1,
         b"the environment tail overlaps the level"),
        # the environment lookups
        ("deferred_light environment", lambda: lit.light("", (), flags=1 | (2 << 16) | 0x8000)[0], -4, DERIVATIVE),
        ("hot path environment", lambda: hot(flags=1 | (2 << 16) | 0x8000), -4, DERIVATIVE),
    ]


@pytest.mark.gpu
def test_refusals_keep_status_and_message(lit, built_lib):
    for what, call, status, message in _refusals(lit, built_lib):
        rc = call()
        assert rc == status, (what, rc, lit.lib.crychic_last_error())
        assert lit.lib.crychic_last_error() == message, what
    torch.cuda.synchronize()
