"""crychic_set_cube_probe_volume and the lighting entries with CRYCHIC_LIGHT_CUBE_PARALLAX on the device against the checker
(tests/parallax_ref) bit for bit: the 48 bytes between canaries, over the previous call's output, on a side stream, in a captured
graph, untouched by the SH projection; every entry and Crychic.Draw over the four ambient x specular combinations, the plane formats,
row strips, the fuzz planes, the frame on which the flag bites, the refusals, and capture_environment(probe_box=...)."""
import ctypes as C

import numpy as np
import pytest

import env_brdf_lib
import env_sh_lib
import gloss_lib
import parallax_lib
from env_brdf_lib import ENV_BRDF
from env_sh_lib import AMBIENT_SH
from parallax_lib import PARALLAX, PROBE_BYTES, PROBE_OFFSET, probe_floats, probe_offset, with_probe
from test_env_brdf_host import eye_of, random_table, with_eye, with_table_roughness, with_view_normals
from test_env_sh_host import scene_block
from test_gloss_host import GLOSS, SIZES, gloss_chain, levels_flag, same_frame
from test_parallax_host import (BITES_DIM, BITES_LEVELS, BITES_PROBE, BOX, COMBOS, FACE_COLOURS, bites_frame, box_flags, face_chain,
                                scene_probe)

pytestmark = pytest.mark.gpu

GUARD = 256
TAIL = 512


@pytest.fixture(scope="module")
def px():
    return parallax_lib.load()


@pytest.fixture(scope="module")
def eb():
    return env_brdf_lib.load()


@pytest.fixture(scope="module")
def es():
    return env_sh_lib.load()


@pytest.fixture(scope="module")
def gl():
    return gloss_lib.load()


@pytest.fixture(scope="module")
def ctx(built_lib):
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


# ---- the setter --------------------------------------------------------------------------------------------------------------------------

def _set(ctx, buf, off, volume, stream=None):
    import torch
    from crychic_renderer_amd import lib
    from crychic_renderer_amd._lib import check
    st = torch.cuda.current_stream(ctx.device) if stream is None else stream
    v = [(C.c_float * 3)(*[float(x) for x in a]) for a in volume]
    check(lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(buf.data_ptr() + off), v[0], v[1], v[2], C.c_void_p(st.cuda_stream)))
    return st


def _tail(ctx, fill=0xA5, shift=0):
    """[GUARD + shift of 0xA5][a 512-byte tail of `fill`][GUARD of 0xA5] on the device: (tensor, host copy, tail offset)."""
    import torch
    off = GUARD + shift
    host = np.full(off + TAIL + GUARD, 0xA5, np.uint8)
    host[off:off + TAIL] = fill
    buf = torch.from_numpy(host.copy()).to(ctx.device)
    assert buf.data_ptr() % 16 == 0
    return buf, host, off


def _check_volume(got, host, off, volume):
    """Tail bytes [368, 416) are the twelve floats, everything else is untouched."""
    lo = off + PROBE_OFFSET
    assert np.array_equal(np.frombuffer(got[lo:lo + PROBE_BYTES].tobytes(), np.uint32), probe_floats(*volume).view(np.uint32))
    keep = np.ones(got.size, bool)
    keep[lo:lo + PROBE_BYTES] = False
    assert np.array_equal(got[keep], host[keep])


OTHER = ((-7.5, 4.0, 9.0), (-30.0, 0.0, -12.0), (-1.0, 9.0, 40.0))


def test_volume_between_canaries_and_over_its_own_output(ctx):
    import torch
    buf, host, off = _tail(ctx)
    _set(ctx, buf, off, BOX).synchronize()
    first = buf.cpu().numpy()
    _check_volume(first, host, off, BOX)
    _set(ctx, buf, off, BOX).synchronize()
    assert np.array_equal(buf.cpu().numpy(), first)
    _set(ctx, buf, off, OTHER).synchronize()
    _check_volume(buf.cpu().numpy(), host, off, OTHER)
    # a tail that is only 4-byte aligned
    buf, host, off = _tail(ctx, fill=0xFF, shift=4)
    assert (buf.data_ptr() + off) % 8 == 4
    _set(ctx, buf, off, OTHER).synchronize()
    _check_volume(buf.cpu().numpy(), host, off, OTHER)
    torch.cuda.synchronize()


def test_volume_runs_on_the_callers_stream(ctx):
    """The tail is filled with 0xFF on a side stream behind other work and the setter is enqueued on that stream: launched on any other
    it would be overwritten by the fill."""
    import torch
    buf, host, off = _tail(ctx, fill=0x00)
    ballast = torch.empty((1 << 28,), dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=ctx.device)
    with torch.cuda.stream(side):
        for k in range(16):
            ballast.fill_(k)
        buf[off:off + TAIL].fill_(0xFF)
    _set(ctx, buf, off, BOX, stream=side)
    side.synchronize()
    host[off:off + TAIL] = 0xFF
    _check_volume(buf.cpu().numpy(), host, off, BOX)


def test_volume_captured_into_a_graph_and_replayed(ctx):
    """Nothing is allocated or copied from the host at replay: the twelve floats were captured with the kernel's arguments."""
    import torch
    buf, host, off = _tail(ctx, fill=0xFF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _set(ctx, buf, off, OTHER)
    for fill in (0x00, 0x5A):
        buf[off:off + TAIL].fill_(fill)
        host[off:off + TAIL] = fill
        graph.replay()
        torch.cuda.synchronize()
        _check_volume(buf.cpu().numpy(), host, off, OTHER)


def test_the_sh_projection_leaves_the_volume_and_the_reserved_bytes_alone(built_lib, ctx):
    """crychic_project_cube_sh after the setter writes tail bytes [0, 368) only."""
    import torch
    from crychic_renderer_amd import lib
    d = 16
    level = torch.from_numpy(np.random.default_rng(4).integers(0, 256, 6 * d * d * 4, dtype=np.uint8)).to(ctx.device)
    buf, host, off = _tail(ctx)
    _set(ctx, buf, off, BOX)
    st = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    built_lib.check(lib.crychic_project_cube_sh(ctx.handle, C.c_void_p(level.data_ptr()), d, C.c_void_p(buf.data_ptr() + off), st))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    lo = off + PROBE_OFFSET
    assert np.array_equal(got[lo:lo + PROBE_BYTES].view(np.uint32), probe_floats(*BOX).view(np.uint32))
    assert (got[off + 416:off + TAIL] == 0xA5).all() and (got[:off] == 0xA5).all() and (got[off + TAIL:] == 0xA5).all()
    assert (got[off:off + 144] != 0xA5).any()               # the projection did run


def test_volume_argument_errors(ctx):
    import torch
    from crychic_renderer_amd import lib
    buf, host, off = _tail(ctx)
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    a = buf.data_ptr() + off
    f3 = lambda v: (C.c_float * 3)(*v)
    c, lo, hi = (f3(v) for v in BOX)
    assert lib.crychic_set_cube_probe_volume(ctx.handle, None, c, lo, hi, st) == -1
    assert lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(a), None, lo, hi, st) == -1
    assert lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(a), c, None, hi, st) == -1
    assert lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(a), c, lo, None, st) == -1
    assert lib.crychic_set_cube_probe_volume(None, C.c_void_p(a), c, lo, hi, st) == -1
    for mis in (1, 2, 3):
        assert lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(a + mis), c, lo, hi, st) == -1 and b"4-byte" in lib.crychic_last_error()
    for bad in (f3((np.nan, 0, 0)), f3((0, np.inf, 0)), f3((4, 0, 0)), f3((0, -2, 0)), f3((0, 0, 5))):
        assert lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(a), bad, lo, hi, st) == -1 and b"boxMin < pos < boxMax" in lib.crychic_last_error()
    assert lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(a), c, f3((-4, -np.inf, -4)), hi, st) == -1
    assert lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(a), c, lo, f3((4, np.nan, 4)), st) == -1
    assert lib.crychic_set_cube_probe_volume(ctx.handle, C.c_void_p(a), c, hi, lo, st) == -1
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), host)          # the refused calls enqueued nothing


# ---- the lighting pass on the device -------------------------------------------------------------------------------------------------

from test_gloss_gpu import ENTRIES, _call, _dev_planes, _frames_equal, _to_dev  # noqa: E402


def _cube(chain, dim, levels, k, block, eb, spec, table=None):
    return with_probe(chain, dim, levels, scene_probe(k), block, (eb.table()[0] if table is None else table) if spec else None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_lighting_entry_with_the_flag_equals_the_checker(built_lib, ctx, px, eb, es, gl, entry):
    """Each crychic_deferred_light* entry with CRYCHIC_LIGHT_CUBE_PARALLAX == the checker, RGBA8 and radiance bits, over the four ambient
    x specular combinations, each at 64 x 48 (2 levels) and 70 x 38 (5 levels), each with radius 0 and a radius > 0 (with the Q fixes),
    with the lights and the shadows the entry takes and three probe volumes; the roughness and normal edge values."""
    import torch
    from local_lights_util import FIX_ALL, _dev_lights
    from test_point_shadows import _frame_setup, _point_desc, _spot_desc
    for n, ((W, H), levels) in enumerate(zip(SIZES, (2, 5))):
        p, cb, pcb, spots, points, maps, cubes, projs = _frame_setup(W, H, 2, 48, 3, seed=3 + levels)
        chain, dim = gloss_chain(gl, p, levels)
        q = with_view_normals(with_table_roughness(p, levels), eye_of(cb))
        block = scene_block(es, p)
        kw, dkw = {}, {}
        if entry != "light":
            kw["points"], dkw["points"] = points, _dev_lights(ctx, points)
        if entry in ("spots", "spots_shadowed", "point_shadows"):
            kw["spots"], dkw["spots"] = spots, _dev_lights(ctx, spots)
        if entry in ("spots_shadowed", "point_shadows"):
            mdev = _to_dev(ctx, maps)
            kw["maps"], dkw["sdesc"] = maps, _spot_desc(mdev)
        if entry == "point_shadows":
            cdev = _to_dev(ctx, cubes)
            kw["cubes"], kw["projs"], dkw["pdesc"] = cubes, projs, _point_desc(cdev, projs)
        for k, (sh, spec) in enumerate(COMBOS):
            qq = dict(q, cube=_cube(chain, dim, levels, k + n, block, eb, spec, random_table(9) if n else None))
            dev = _dev_planes(ctx, qq)
            for radius, fixes in ((0.0, 0), (0.01, FIX_ALL)):
                flags = fixes | 1 | box_flags(levels, sh, spec)
                rc, out, rad = _call(built_lib.lib, ctx, entry, cb, dev, W, H, flags, dim, radius=radius, **dkw)
                built_lib.check(rc)
                torch.cuda.synchronize()
                ref = px.checker_light(pcb, qq, None, 3, radius, flags, cube_dim=dim, **kw)
                assert _frames_equal(out, rad, ref), (entry, W, H, sh, spec, radius)


def test_half_float_planes_and_an_infinite_eye(built_lib, ctx, px, eb, es, gl):
    """The `mixed` and the all-half planes: the device on the packed planes == the checker on the widened ones; then float planes with an
    infinite EyePosW."""
    import torch
    import gbuffer_f16_lib as gf
    from local_lights_util import _cpu
    W, H = SIZES[1]
    _, p, c, pcb = _cpu(W, H)
    for n, (levels, (sh, spec)) in enumerate(zip((2, 5, 5, 2), COMBOS)):
        chain, dim = gloss_chain(gl, p, levels)
        q = dict(with_view_normals(with_table_roughness(p, levels), eye_of(c.pass_cb)), cube=_cube(chain, dim, levels, n, scene_block(es, p), eb, spec))
        flags = 1 | box_flags(levels, sh, spec)
        for mix in (gf.MIXED, gf.F16_MASK):
            packed = gf.pack_planes(q, mix)
            wide = gf.widen_planes(packed)
            rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, packed), W, H, flags | mix, dim)
            built_lib.check(rc)
            torch.cuda.synchronize()
            assert _frames_equal(out, rad, px.checker_light(pcb, wide, None, 3, 0.0, flags, cube_dim=dim)), (n, hex(mix))
        cb2, pcb2 = with_eye(c.pass_cb, (np.inf, 3.0, -np.inf))
        rc, out, rad = _call(built_lib.lib, ctx, "light", cb2, _dev_planes(ctx, q), W, H, flags, dim, radius=0.01)
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, px.checker_light(pcb2, q, None, 3, 0.01, flags, cube_dim=dim)), n


def test_frame_in_three_row_strips_with_an_odd_row0(built_lib, ctx, px, eb, es, gl):
    """128 x 96 lit as rows [0, 31), [31, 64), [64, 96) equals the whole frame's checker: gloss needs no quad rows."""
    import torch
    from local_lights_util import _cpu
    W, H = 128, 96
    _, p, c, pcb = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, 5)
    q = with_view_normals(with_table_roughness(p, 5), eye_of(c.pass_cb))
    for k, (sh, spec) in enumerate(COMBOS[1:3]):
        qq = dict(q, cube=_cube(chain, dim, 5, k, scene_block(es, p), eb, spec))
        dev = _dev_planes(ctx, qq)
        flags = 1 | box_flags(5, sh, spec)
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
        rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
        for r0, r1 in ((0, 31), (31, 64), (64, 96)):
            rc, _, _ = _call(built_lib.lib, ctx, "light", c.pass_cb, dev, W, H, flags, dim, row0=r0, rows=r1 - r0, out=out, rad=rad)
            built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, px.checker_light(pcb, qq, None, 3, 0.0, flags, cube_dim=dim)), (sh, spec)


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_fuzz_planes_on_the_device(built_lib, ctx, px, eb, es, seed):
    import torch
    import fuzz_util
    import oracle_lib
    from crychic_renderer_amd import geometry as g
    W, H, planes, c, knobs = fuzz_util.random_case(seed, built_lib)
    chain, levels = g.cube_mip_chain(planes["cube"])
    dim = planes["cube"].shape[1]
    pcb = oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
    block = es.project(planes["cube"])
    for k, (sh, spec) in enumerate(COMBOS):
        q = dict(planes, cube=with_probe(chain, dim, levels, scene_probe(seed + k), block, random_table(seed) if spec else None))
        flags = knobs["sky"] | box_flags(levels, sh, spec)
        rc, out, rad = _call(built_lib.lib, ctx, "light", c.pass_cb, _dev_planes(ctx, q), W, H, flags, dim, ndl=knobs["numDirLights"],
                             radius=knobs["pcfSearchRadius"])
        built_lib.check(rc)
        torch.cuda.synchronize()
        assert _frames_equal(out, rad, px.checker_light(pcb, q, None, knobs["numDirLights"], knobs["pcfSearchRadius"], flags, cube_dim=dim)), (sh, spec)


def test_the_flag_bites_on_the_device(built_lib, ctx, px, gl):
    """The hand-built frame of tests/test_parallax_host.py: without the flag the device reflects the +Y face, with it the +X face, each
    the checker's frame bit for bit, and the two differ on every pixel."""
    import torch
    planes, c, eye = bites_frame()
    cb, pcb = with_eye(c.pass_cb, eye)
    H, W = planes["depth"].shape
    host = dict(planes, cube=with_probe(face_chain(FACE_COLOURS), BITES_DIM, BITES_LEVELS, probe_floats(*BITES_PROBE)))
    dev = _dev_planes(ctx, host)
    base = GLOSS | levels_flag(BITES_LEVELS)
    frames = []
    for flags in (base, base | PARALLAX):
        rc, out, rad = _call(built_lib.lib, ctx, "light", cb, dev, W, H, flags, BITES_DIM, ndl=1)
        built_lib.check(rc)
        torch.cuda.synchronize()
        frames.append((out.cpu().numpy(), rad.cpu().numpy()))
    all_x, all_y = face_chain(FACE_COLOURS[[0] * 6]), face_chain(FACE_COLOURS[[2] * 6])
    assert same_frame(frames[0], gl.checker_light(pcb, dict(planes, cube=all_y), None, 1, 0.0, base, cube_dim=BITES_DIM))
    assert same_frame(frames[1], gl.checker_light(pcb, dict(planes, cube=all_x), None, 1, 0.0, base, cube_dim=BITES_DIM))
    assert same_frame(frames[1], px.checker_light(pcb, host, None, 1, 0.0, base | PARALLAX, cube_dim=BITES_DIM))
    assert (frames[0][0] != frames[1][0]).any(axis=-1).all()


def test_refusals_leave_the_output_untouched(built_lib, ctx, px, eb, es, gl):
    """The flag without CRYCHIC_LIGHT_CUBE_GLOSS or without a chain, a NULL cube map and a misaligned probe volume are
    CRYCHIC_E_INVALID_ARG with their messages, before anything is enqueued: the output keeps its canary fill.  set_cube_map refuses the
    flag without gloss and a tensor without room for the tail."""
    import torch
    from crychic_renderer_amd import Crychic, CrychicError
    from local_lights_util import _cpu
    W, H = SIZES[0]
    _, p, c, _ = _cpu(W, H)
    chain, dim = gloss_chain(gl, p, 5)
    q = dict(p, cube=_cube(chain, dim, 5, 0, scene_block(es, p), eb, True))
    dev = _dev_planes(ctx, q)
    lib = built_lib.lib
    out = torch.full((H, W, 4), 0xA5, dtype=torch.uint8, device=ctx.device)
    rad = torch.full((H, W, 4), -7.0, dtype=torch.float32, device=ctx.device)
    for entry in ENTRIES:
        for flags in (1 | PARALLAX | levels_flag(5), 1 | PARALLAX, 1 | PARALLAX | AMBIENT_SH, 1 | PARALLAX | levels_flag(1)):
            rc, _, _ = _call(lib, ctx, entry, c.pass_cb, dev, W, H, flags, dim, out=out, rad=rad)
            assert rc == -1 and b"CRYCHIC_LIGHT_CUBE_PARALLAX needs a prefiltered chain" in lib.crychic_last_error(), (entry, hex(flags))
        for flags in (1 | PARALLAX | GLOSS, 1 | PARALLAX | ENV_BRDF | GLOSS | levels_flag(1)):      # the gloss flag's own refusal comes first
            rc, _, _ = _call(lib, ctx, entry, c.pass_cb, dev, W, H, flags, dim, out=out, rad=rad)
            assert rc == -1 and b"CRYCHIC_LIGHT_CUBE_GLOSS needs a chain" in lib.crychic_last_error(), (entry, hex(flags))
        rc, _, _ = _call(lib, ctx, entry, c.pass_cb, dict(dev, cube=None), W, H, 1 | box_flags(5), dim, out=out, rad=rad)
        assert rc == -1 and b"null argument" in lib.crychic_last_error()      # the entries' own pointer test comes first
        rc, _, _ = _call(lib, ctx, entry, c.pass_cb, dict(dev, cube=dev["cube"][2:]), W, H, 1 | box_flags(5), dim, out=out, rad=rad)
        assert rc == -1 and b"CRYCHIC_LIGHT_CUBE_PARALLAX: the probe volume at cube_dev + %d is not 4-byte aligned" % probe_offset(dim, 5) in lib.crychic_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and (rad.cpu().numpy() == -7.0).all()
    app = Crychic(ctx, W, H, _to_dev(ctx, p["randvec"]), _to_dev(ctx, p["cube"]), shadow_dim=256)
    with pytest.raises(CrychicError, match="parallax needs a tensor of"):
        app.set_cube_map(_to_dev(ctx, chain), dim, 5, gloss=True, parallax=True)          # no room for the tail
    with pytest.raises(CrychicError, match="parallax needs a prefiltered chain"):
        app.set_cube_map(dev["cube"], dim, 5, parallax=True)                              # the flag without gloss
    assert not app.frame_desc().flags & PARALLAX
    app.set_cube_map(dev["cube"], dim, 5, gloss=True, parallax=True)
    assert app.frame_desc().flags & PARALLAX and not app.frame_desc().flags & (AMBIENT_SH | ENV_BRDF)
    app.set_cube_map(dev["cube"], dim, 5, gloss=True)
    assert not app.frame_desc().flags & PARALLAX
    # the hot path refuses the same before it enqueues anything
    app.set_cube_map(_to_dev(ctx, p["cube"]))
    app.flags = PARALLAX
    app.mBackBuffer.fill_(0xA5)
    torch.cuda.synchronize()
    with pytest.raises(CrychicError, match="CRYCHIC_LIGHT_CUBE_PARALLAX needs a prefiltered chain"):
        app.Draw()
    torch.cuda.synchronize()
    assert (app.mBackBuffer.cpu().numpy() == 0xA5).all()


@pytest.mark.parametrize("sh,spec", COMBOS)
def test_hot_path_with_the_flag_equals_the_checker(built_lib, ctx, px, eb, es, gl, sh, spec):
    """Crychic.set_probe_volume into the chain's own tensor, set_cube_map(parallax=True) and Draw (crychic_draw_hot_path): the frame ==
    the checker's, lit with the ambient map the device produced; it differs from the frame without the flag, and Draw's cache key holds
    the state."""
    import torch
    from crychic_renderer_amd import geometry as g
    from local_lights_util import _app, _cpu
    W, H = SIZES[int(sh)]
    pl, p, c, pcb = _cpu(W, H)
    levels = 5 if spec else 2
    chain, dim = gloss_chain(gl, p, levels)
    q = with_view_normals(with_table_roughness(p, levels), eye_of(c.pass_cb))
    block = scene_block(es, p)
    volume = ((0.0, 3.0, 0.0), (-25.0, -1.0, -25.0), (25.0, 18.0, 25.0))
    host = with_probe(chain, dim, levels, np.full(12, np.nan, np.float32), block, eb.table()[0])
    dev = {k: _to_dev(ctx, v) for k, v in dict(q, cube=host).items()}
    app = _app(ctx, W, H, dev, c)
    app.set_cube_map(dev["cube"], dim, levels, gloss=True, ambient_sh=sh, env_brdf=spec)
    app.Draw()
    torch.cuda.synchronize()
    plain = app.mBackBuffer.cpu().numpy().copy()
    assert app.set_probe_volume(dev["cube"], dim, levels, *volume) is dev["cube"]
    app.set_cube_map(dev["cube"], dim, levels, gloss=True, ambient_sh=sh, env_brdf=spec, parallax=True)
    app.Draw()
    torch.cuda.synchronize()
    got = dev["cube"].cpu().numpy()
    off = g.cube_probe_offset(dim, levels)
    assert off == probe_offset(dim, levels) and np.array_equal(got[off:off + PROBE_BYTES].view(np.uint32), probe_floats(*volume).view(np.uint32))
    keep = np.ones(got.size, bool)
    keep[off:off + PROBE_BYTES] = False
    assert np.array_equal(got[keep], host[keep])
    ao = app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16)
    ref = px.checker_light(pcb, dict(q, cube=got), ao, 3, float(app.pcfSearchRadius), 1 | box_flags(levels, sh, spec), cube_dim=dim)
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), ref[0])
    assert (plain != ref[0]).any()
    app.set_cube_map(dev["cube"], dim, levels, gloss=True, ambient_sh=sh, env_brdf=spec)
    app.Draw()
    torch.cuda.synchronize()
    assert np.array_equal(app.mBackBuffer.cpu().numpy(), plain)


def test_capture_environment_with_a_probe_box(built_lib, ctx, px):
    """capture_environment(prefilter=True, env_brdf=True, probe_box=...) writes the capture's own position and the box into the tail of
    the prefiltered chain it returns; set_cube_map(parallax=True) and Draw give the checker's frame over the downloaded chain and planes,
    and another frame than without the flag; probe_box without prefilter is refused."""
    import torch
    import oracle_lib
    import raster_util
    from crychic_renderer_amd import CrychicError, LIGHT_SKY, geometry as g
    from test_env_capture import PROBE, SD, _Scene
    cap = _Scene(ctx)
    app = cap.app(ctx)
    dim = 16
    box = ((0.25, -0.5, 0.25), (4.75, 6.0, 4.75))
    chain, d, levels = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, prefilter=True, env_brdf=True, probe_box=box)
    torch.cuda.synchronize()
    got = chain.cpu().numpy()
    assert (d, levels) == (dim, 5) and got.size == g.cube_chain_env_bytes(dim, levels)
    off = g.cube_probe_offset(dim, levels)
    assert np.array_equal(got[off:off + PROBE_BYTES].view(np.uint32), probe_floats(PROBE, *box).view(np.uint32))
    plain, _, _ = app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, prefilter=True, probe_box=box)
    torch.cuda.synchronize()
    assert plain.numel() == g.cube_chain_sh_bytes(dim, levels)
    assert np.array_equal(plain.cpu().numpy()[off:off + PROBE_BYTES], got[off:off + PROBE_BYTES])
    with pytest.raises(CrychicError, match="probe_box needs prefilter=True"):
        app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, probe_box=box)
    with pytest.raises(CrychicError, match=r"probe_box needs a chain \(levels > 1\)"):
        app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, levels=1, prefilter=True, probe_box=box)
    with pytest.raises(CrychicError):
        app.capture_environment(PROBE, cap.geo, cap.shadow_geo, dim=dim, shadow_dim=SD, prefilter=True, probe_box=(box[1], box[0]))
    app.flags = LIGHT_SKY
    cbs = []
    for k in range(4):
        cb = built_lib.PassConstants()
        cb.ViewProj[:] = list(raster_util.light_viewproj_t(cap.consts, k))
        cbs.append(cb)
    cap.shadow_geo.DrawSceneToShadowMaps(cbs, [app.mShadowMap.Resource(k) for k in range(4)])
    cap.geo.DrawNormalsDepthAndGBuffer(cap.consts.pass_cb, app.mSsao.mNormalMap, app.mDeferred.mGBuffer, app.mDepthStencilBuffer)
    app.set_cube_map(chain, dim, levels, gloss=True, env_brdf=True)
    app.Draw()
    torch.cuda.synchronize()
    without = app.mBackBuffer.cpu().numpy().copy()
    app.set_cube_map(chain, dim, levels, gloss=True, env_brdf=True, parallax=True)
    app.Draw()
    torch.cuda.synchronize()
    frame = app.mBackBuffer.cpu().numpy()
    assert (frame != without).any()
    host = {"g%d" % k: app.mDeferred.mGBuffer[k].cpu().numpy() for k in range(3)}
    host["depth"] = app.mDepthStencilBuffer.cpu().numpy().view(np.uint32)
    host["shadow"] = app.mShadowMap.mShadowMap.cpu().numpy().view(np.uint32)
    host["cube"] = got
    ao = app.mSsao.mAmbientMap0.cpu().numpy().view(np.uint16)
    pcb = oracle_lib.as_oracle_cb(app.mMainPassCB, oracle_lib.OrPassConstants)
    flags = int(app.flags) | box_flags(levels, False, True)
    assert app.frame_desc().flags == flags
    ref = px.checker_light(pcb, host, ao, int(app.numDirLights), float(app.pcfSearchRadius), flags, cube_dim=dim)
    assert np.array_equal(frame, ref[0])
