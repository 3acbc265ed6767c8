"""Producer passes on triangle soups, device tier: the HIP rasteriser through the C ABI against the oracle, bit for
bit on every plane, on the cases of raster_soup_lib.  What exists only in raster.hip is the subject: the batch lookup of the setup
kernel (more than eight items, empty items, both draw-item locations, slots carried over batches and fused targets), serials as the
tie-break of the atomic minimum, the two ends of the live list with boxes right at the split, the clears' odd tails and unaligned
heads, fp64 depth on steep slivers, and clipped primitives through every resolve.  test_raster_soup_host.py shows the cases meet
their conditions; every test here also wants crychic_raster_status == 0."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_f16_lib as gf
import oracle_lib
import raster_soup_lib as soup

torch = pytest.importorskip("torch")

DEPTH_POISON, NORMAL_POISON, G_POISON, CANARY = 0x12345, 0x5A5A, 0x7FC01234, 0x0BADF00D
BIASES = ((10000, 2.0), (0, 0.0))


@pytest.fixture(scope="module")
def ctx(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    _GEO.clear()
    c.close()


_GEO, _REF = {}, {}


def geometry(ctx, case):
    from crychic_renderer_amd import SceneGeometry
    if case["name"] not in _GEO:
        _GEO[case["name"]] = SceneGeometry(ctx, case["items"], case["materials"], case["textures"])
    return _GEO[case["name"]]


def reference(oracle, case, mode, bias=(0, 0.0), viewproj=None, size=None):
    """The oracle's planes, computed once per (case, pass, bias, ViewProj, target size).  size: (W, H); default the case's frame for
    modes 1 and 2, its square shadow target for mode 0."""
    vp = case["viewproj"] if viewproj is None else np.ascontiguousarray(viewproj, np.float32).reshape(16)
    W, H = size or ((case["W"], case["H"]) if mode else (case["shadow_dim"],) * 2)
    key = (case["name"], mode, bias, vp.tobytes(), W, H)
    if key not in _REF:
        r = oracle_lib.rasterize(oracle, mode, case["view"], vp, case["items"], case["materials"], case["textures"], W, H, *bias)
        for k in ("normal", "g0", "g1", "g2"):
            assert r[k] is None or np.isfinite(r[k].astype(np.float32)).all(), k
        _REF[key] = r
    return _REF[key]


def pass_cb(built_lib, case, viewproj=None):
    cb = built_lib.PassConstants()
    cb.View[:] = [float(x) for x in case["view"]]
    cb.ViewProj[:] = [float(x) for x in (case["viewproj"] if viewproj is None else np.asarray(viewproj, np.float32).reshape(16))]
    return cb


def status(ctx, built_lib):
    flags = C.c_uint32(99)
    built_lib.check(built_lib.lib.crychic_raster_status(ctx.handle, None, C.byref(flags)))
    return flags.value


def poisoned(ctx, W, H, half=(False, False, False)):
    """Fresh targets full of values no pass writes: depth (H, W) int32, normal (H, W, 4) fp16, G0..G2 (H, W, 4) fp32 or fp16."""
    dev = ctx.device
    depth = torch.full((H, W), DEPTH_POISON, dtype=torch.int32, device=dev)
    normal = torch.full((H, W, 4), NORMAL_POISON, dtype=torch.int16, device=dev).view(torch.float16)
    g = [torch.full((H, W, 4), NORMAL_POISON, dtype=torch.int16, device=dev).view(torch.float16) if h else
         torch.full((H, W, 4), G_POISON, dtype=torch.int32, device=dev).view(torch.float32) for h in half]
    return depth, normal, g


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(got, ref):
    return np.array_equal(bits(got), bits(ref))


def run_pass(ctx, built_lib, geo, cb, which, W, H, rows=None, half=(False, False, False)):
    """One producer pass into freshly poisoned targets; returns {plane: numpy bits}."""
    depth, normal, g = poisoned(ctx, W, H, half)
    if which == "normals":
        geo.DrawNormalsAndDepth(cb, normal, depth)
    elif which == "gbuffer":
        geo.DrawGBuffer(cb, g, depth, g_rows=rows)
    else:
        geo.DrawNormalsDepthAndGBuffer(cb, normal, g, depth, g_rows=rows)
    assert status(ctx, built_lib) == 0, which
    out = {"depth": bits(depth)}
    if which != "gbuffer":
        out["normal"] = bits(normal)
    if which != "normals":
        out.update({"g%d" % k: bits(g[k]) for k in range(3)})
    return out


def check_planes(out, nd, gb, where=""):
    for k, v in out.items():
        ref = nd if k == "normal" else gb
        assert np.array_equal(v, bits(ref[k])), (where, k, int((v != bits(ref[k])).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", soup.CASE_NAMES)
def test_every_pass_matches_the_oracle(ctx, built_lib, oracle, name):
    """Normals + depth, the G-buffer, the fused pass and the shadow pass with and without its bias; each issued twice into fresh
    targets: equal to each other and to the oracle."""
    case = soup.get(name)
    geo, cb, W, H = geometry(ctx, case), pass_cb(built_lib, case), case["W"], case["H"]
    nd, gb = reference(oracle, case, 1), reference(oracle, case, 2)
    assert np.array_equal(nd["depth"], gb["depth"])
    for which in ("normals", "gbuffer", "fused"):
        first, second = (run_pass(ctx, built_lib, geo, cb, which, W, H) for _ in range(2))
        assert all(np.array_equal(first[k], second[k]) for k in first), which
        check_planes(first, nd, gb, which)
    dim = case["shadow_dim"]
    for bias in BIASES:
        ref = reference(oracle, case, 0, bias)
        maps = []
        for _ in range(2):
            m = torch.full((dim, dim), DEPTH_POISON, dtype=torch.int32, device=ctx.device)
            geo.DrawSceneToShadowMap(cb, m, *bias)
            assert status(ctx, built_lib) == 0
            maps.append(bits(m))
        assert np.array_equal(maps[0], maps[1]) and np.array_equal(maps[0], ref["depth"]), (bias, int((maps[0] != ref["depth"]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["threshold-" + v for v in soup.THRESHOLD] + ["clip"])
def test_scissor_rows(ctx, built_lib, oracle, name):
    """Strip-limited G-buffer passes: inside the rows the planes equal the unscissored oracle; outside them the poison survives in
    G0..G2, and in depth too for the G-buffer-only entry (whose rasterisation is limited to the rows: large triangles start
    mid-stripe).  The fused entry still renders depth and normals for the whole frame."""
    case = soup.get(name)
    geo, cb, W, H = geometry(ctx, case), pass_cb(built_lib, case), case["W"], case["H"]
    nd, gb = reference(oracle, case, 1), reference(oracle, case, 2)
    for r0, rn in ((1, 5), (H - 1, 1), (H // 2 - 3, 7), (0, H)):
        inside = np.zeros(H, bool); inside[r0:r0 + rn] = True
        for which in ("gbuffer", "fused"):
            out = run_pass(ctx, built_lib, geo, cb, which, W, H, rows=(r0, rn))
            for k in ("g0", "g1", "g2"):
                assert np.array_equal(out[k][inside], bits(gb[k])[inside]), (which, r0, rn, k)
                assert (out[k][~inside] == G_POISON).all(), (which, r0, rn, k)
            if which == "gbuffer":
                assert np.array_equal(out["depth"][inside], gb["depth"][inside]) and (out["depth"][~inside] == DEPTH_POISON).all(), (r0, rn)
            else:
                assert np.array_equal(out["depth"], nd["depth"]) and np.array_equal(out["normal"], bits(nd["normal"])), (r0, rn)


def sheared(case, k):
    """ViewProj of fused target k: the case's own (k = 0), or scaled and sheared in clip-space x and y."""
    s = np.eye(4, dtype=np.float32)
    if k:
        s[0, 0], s[0, 1], s[1, 0], s[1, 1] = 1.0 - 0.17 * k, 0.11 * k, -0.07 * k, 1.0 + 0.09 * k
    return (s @ case["viewproj"].reshape(4, 4)).astype(np.float32).reshape(16)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4, 5])
@pytest.mark.parametrize("name", ["clip", "threshold-square"])
def test_fused_cascades(ctx, built_lib, oracle, name, n):
    """crychic_draw_scene_to_shadow_maps with n targets, each under its own ViewProj (five run as 4 + 1): every target equals the
    oracle's single pass for its ViewProj."""
    case = soup.get(name)
    geo, dim = geometry(ctx, case), case["shadow_dim"]
    vps = [sheared(case, k) for k in range(n)]
    maps = [torch.full((dim, dim), DEPTH_POISON, dtype=torch.int32, device=ctx.device) for _ in range(n)]
    geo.DrawSceneToShadowMaps([pass_cb(built_lib, case, vp) for vp in vps], maps)
    assert status(ctx, built_lib) == 0
    for k in range(n):
        ref = reference(oracle, case, 0, BIASES[0], viewproj=vps[k])
        assert same(maps[k], ref["depth"]), (k, int((bits(maps[k]) != ref["depth"]).sum()))
    assert len({reference(oracle, case, 0, BIASES[0], viewproj=vp)["depth"].tobytes() for vp in vps}) == n     # the targets differ


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 3, 33, 95])
def test_shadow_targets_of_any_size_and_alignment(ctx, built_lib, oracle, dim):
    """Shadow planes of odd sizes placed 0, 1, 2 and 3 dwords into a larger allocation (clear_depth_kernel's head and tail): the
    plane equals the oracle and the dwords on both sides of it survive.  `stack` leaves part of the map at the clear value."""
    lib = built_lib.lib
    guard = 8
    for name in ("stack", "clip"):
        case = soup.get(name)
        geo, cb = geometry(ctx, case), pass_cb(built_lib, case)
        ref = reference(oracle, case, 0, BIASES[0], size=(dim, dim))["depth"]
        ws = geo.workspace(dim, dim)
        for off in range(4):
            buf = torch.full((guard + off + dim * dim + guard,), CANARY, dtype=torch.int32, device=ctx.device)
            assert buf.data_ptr() % 16 == 0
            built_lib.check(lib.crychic_draw_scene_to_shadow_map(ctx.handle, C.byref(cb), geo.items, len(geo.items),
                                                                 C.c_void_p(buf.data_ptr() + 4 * (guard + off)), dim, BIASES[0][0], BIASES[0][1],
                                                                 C.c_void_p(ws.data_ptr()), ws.numel(), None))
            assert status(ctx, built_lib) == 0
            got = bits(buf)
            assert np.array_equal(got[guard + off:guard + off + dim * dim].reshape(dim, dim), ref), (name, off)
            assert (got[:guard + off] == CANARY).all() and (got[guard + off + dim * dim:] == CANARY).all(), (name, off)
    assert dim < 3 or (ref < 0xFFFFFF).any()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(97, 61), (1, 1), (3, 5)])
def test_frame_targets_with_an_odd_pixel_count(ctx, built_lib, oracle, W, H):
    """clear_vis_kernel's odd tail, and a visibility buffer that ends 8 bytes short of a 16-byte boundary."""
    for name in ("stack", "clip"):
        case = soup.get(name)
        geo, cb = geometry(ctx, case), pass_cb(built_lib, case)
        nd, gb = reference(oracle, case, 1, size=(W, H)), reference(oracle, case, 2, size=(W, H))
        for which in ("normals", "gbuffer", "fused"):
            check_planes(run_pass(ctx, built_lib, geo, cb, which, W, H), nd, gb, (name, which))


@pytest.mark.gpu
@pytest.mark.parametrize("mix", [gf.MIXED, gf.ALL_F16], ids=["mixed", "f16"])
def test_gbuffer_formats_on_clipped_primitives(ctx, built_lib, oracle, mix):
    """crychic_draw_gbuffer_formats on `clip`: a half4 plane holds the oracle's fp32 plane rounded to nearest even (numpy's
    astype(float16), the conversion of float_to_half).  mixed: G0 float4, G1 and G2 half4; f16: all three half4."""
    half = tuple(bool(mix & bit) for bit in (gf.G0_F16, gf.G1_F16, gf.G2_F16))
    case = soup.get("clip")
    geo, cb, W, H = geometry(ctx, case), pass_cb(built_lib, case), case["W"], case["H"]
    nd, gb = reference(oracle, case, 1), reference(oracle, case, 2)
    with np.errstate(over="ignore"):
        expect = dict(gb, **{"g%d" % k: gb["g%d" % k].astype(np.float16) for k in range(3) if half[k]})
    for which in ("gbuffer", "fused"):
        check_planes(run_pass(ctx, built_lib, geo, cb, which, W, H, half=half), nd, expect, which)


@pytest.mark.gpu
def test_bad_triangles_among_good_ones(ctx, built_lib, oracle):
    """`mixed` seed 0 with a triangle whose index lies outside its vertex buffer and one with a NaN position, mid-list and in
    different setup batches: both are reported (status 3) and every plane equals the oracle's render of the soup without them."""
    from crychic_renderer_amd import SceneGeometry
    case = soup.get("mixed-0")
    W, H = case["W"], case["H"]
    v = np.zeros(3, oracle_lib.VERTEX_DT)
    v["Pos"] = [soup.from_ndc(-0.5, -0.5, 3.0, W, H), soup.from_ndc(-0.5, 0.5, 3.0, W, H), soup.from_ndc(0.5, -0.5, 3.0, W, H)]
    v["Normal"] = (0.0, 0.0, -1.0); v["TangentU"] = (1.0, 0.0, 0.0)
    nan = v.copy(); nan["Pos"][2, 0] = np.nan
    inst = soup.make_instances([soup.IDENTITY], [0])
    both = np.array([0, 1, 2, 0, 2, 1], np.uint32)
    items = list(case["items"])
    items.insert(3, (v, np.array([0, 1, 7, 0, 7, 1], np.uint32), inst))
    items.insert(11, (nan, both, inst))
    assert len(items) == 14
    geo = SceneGeometry(ctx, items, case["materials"], case["textures"])
    cb = pass_cb(built_lib, case)
    nd, gb = reference(oracle, case, 1), reference(oracle, case, 2)
    depth, normal, g = poisoned(ctx, W, H)
    geo.DrawNormalsDepthAndGBuffer(cb, normal, g, depth)
    assert status(ctx, built_lib) == 3
    assert same(depth, nd["depth"]) and same(normal, nd["normal"]) and all(same(g[k], gb["g%d" % k]) for k in range(3))
    m = torch.full((case["shadow_dim"],) * 2, DEPTH_POISON, dtype=torch.int32, device=ctx.device)
    geo.DrawSceneToShadowMap(cb, m, *BIASES[0])
    assert status(ctx, built_lib) == 3
    assert same(m, reference(oracle, case, 0, BIASES[0])["depth"])
