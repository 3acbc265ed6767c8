"""The C++ veneer (include/crychic/*.h: CRYCHIC, Ssao, DeferredShading, ShadowMap, FrameResource, UploadBuffer with the
reference's names and call sequence) driven by a native executable, checked against the oracle."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import scene_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "veneer_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "veneer_driver")


def build_driver(name="veneer_driver"):
    """tests/cpp/<name>.cpp -> tests/cpp/<name>, linked against the in-tree libcrychic_hip.so (rebuilt when a header changed)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    src, exe = os.path.join(cpp, name + ".cpp"), os.path.join(cpp, name)
    hdrs = [os.path.join(ROOT, "include", "crychic", f) for f in os.listdir(os.path.join(ROOT, "include", "crychic"))]
    deps = [src, os.path.join(ROOT, "include", "crychic_hip.h")] + hdrs + [os.path.join(cpp, f) for f in os.listdir(cpp) if f.endswith(".hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src,
                        "-L", os.path.join(ROOT, "crychic_renderer_amd"), "-lcrychic_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "crychic_renderer_amd"), "-o", exe], check=True)
    return exe


def run_driver(name, tmp_path, W, H, SD, CD, BC, NL, ok, extra=()):
    """Runs tests/cpp/<name> -- a driver of a post-process pass -- in tmp_path over the W x H built-in scene with the synthetic cube
    map of side CD (`extra`: the arguments behind the seven every such driver takes) and checks its exit code and its `ok` line.
    Returns (the directory, frame), where frame(file name) is an (H, W, 4) uint8 file the driver left there."""
    import torch
    from crychic_renderer_amd import scene
    exe = build_driver(name)
    d = str(tmp_path)
    scene.make_cubemap(CD, torch.device("cpu")).numpy().tofile(d + "/cube.bin")
    r = subprocess.run([exe, d] + [str(v) for v in (W, H, SD, CD, BC, NL) + tuple(extra)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ok in r.stdout
    return d, lambda name: np.fromfile(d + "/" + name, np.uint8).reshape(H, W, 4)


def test_veneer_compiles(built_lib):
    """CPU tier: the veneer headers + driver compile and link against libcrychic_hip.so."""
    assert os.path.exists(build_driver())


@pytest.mark.gpu
def test_veneer_frame_matches_oracle(built_lib, oracle, tmp_path):
    exe = build_driver()
    W, H, SD, CD, BC, NL = 128, 96, 256, 32, 3, 3
    pl = scene_util.cpu_scene(W, H, SD, CD)
    p = scene_util.np_planes(pl)
    d = str(tmp_path)
    p["depth"].tofile(d + "/depth.bin"); p["normal"].tofile(d + "/normal.bin"); p["cube"].tofile(d + "/cube.bin")
    for i in range(3):
        p["g%d" % i].tofile(d + "/g%d.bin" % i)
    for i in range(4):
        p["shadow"][i].tofile(d + "/shadow%d.bin" % i)
    r = subprocess.run([exe, d, str(W), str(H), str(SD), str(CD), str(BC), str(NL)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "veneer ok" in r.stdout
    out = np.fromfile(d + "/out.bin", dtype=np.uint8).reshape(H, W, 4)
    ao = np.fromfile(d + "/ao.bin", dtype=np.uint16).reshape(H // 2, W // 2)
    randvec = np.fromfile(d + "/randvec.bin", dtype=np.uint8).reshape(256, 256, 4)
    # the veneer's Ssao built the MSVC-rand noise texture itself (Ssao.cpp:392-402): same bytes as the host builder
    assert np.array_equal(randvec, pl["consts"].randvec)
    import ctypes as C
    scb, pcb = oracle_lib.OrSsaoConstants(), oracle_lib.OrPassConstants()
    C.memmove(C.addressof(scb), open(d + "/ssao_cb.bin", "rb").read(), C.sizeof(scb))
    C.memmove(C.addressof(pcb), open(d + "/pass_cb.bin", "rb").read(), C.sizeof(pcb))
    assert abs(scb.OcclusionFadeEnd - 1.0) < 1e-7 and pcb.FarZ == 1000.0
    ref_ao = oracle.compute_ssao(scb, p["normal"], p["depth"], randvec, BC)
    assert np.array_equal(ao, ref_ao)
    ref = oracle.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], ref_ao, p["shadow"], p["cube"], NL,
                                built_lib.lib.crychic_pcf_search_radius(SD, 1), sky=True)
    assert np.array_equal(out, ref)


@pytest.mark.gpu
def test_veneer_full_scene_matches_oracle(built_lib, oracle, tmp_path):
    """CRYCHIC::Initialize builds the reference's live scene (100 instanced boxes + grid in one vertex/index buffer with
    BaseVertexLocation / StartIndexLocation), Update fills the instance / material / pass upload buffers, Draw runs the
    producer passes and the hot path: every plane equals the all-CPU oracle frame."""
    import ctypes as C
    import raster_util
    from crychic_renderer_amd import geometry as g, scene
    import torch
    exe = build_driver()
    W, H, SD, CD, BC, NL = 160, 120, 256, 32, 2, 1
    d = str(tmp_path)
    cube = scene.make_cubemap(CD, torch.device("cpu")).numpy()
    cube.tofile(d + "/cube.bin")
    r = subprocess.run([exe, d, str(W), str(H), str(SD), str(CD), str(BC), str(NL), "scene"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    consts = raster_util.frame_constants(W, H, SD)
    # the driver's own constant buffers (same builders, same camera) drive the oracle
    C.memmove(C.addressof(consts.ssao_cb), open(d + "/ssao_cb.bin", "rb").read(), C.sizeof(consts.ssao_cb))
    C.memmove(C.addressof(consts.pass_cb), open(d + "/pass_cb.bin", "rb").read(), C.sizeof(consts.pass_cb))
    # UpdateInstanceData culls against the camera frustum (CRYCHIC.h:188): culled boxes are missing from the shadow pass too
    cam = scene.default_camera(W, H)
    items, shadow_items = g.cascade_scene_items(cull_camera=cam), g.cascade_scene_items(shadow_layer=True, cull_camera=cam)
    assert len(items[0][2]) < 100
    ref = raster_util.oracle_frame(oracle, consts, items, shadow_items, g.reference_materials(),
                                   None, W, H, SD, cube, BC, NL, built_lib.lib.crychic_pcf_search_radius(SD, 1))
    for k in range(4):
        assert np.array_equal(np.fromfile(d + "/shadow%d_out.bin" % k, np.uint32).reshape(SD, SD), ref["shadow"][k]), k
    assert np.array_equal(np.fromfile(d + "/depth_out.bin", np.uint32).reshape(H, W), ref["depth"])
    assert np.array_equal(np.fromfile(d + "/normal_out.bin", np.uint16).reshape(H, W, 4), ref["normal"].view(np.uint16))
    for i, k in enumerate(("g0", "g1", "g2")):
        assert np.array_equal(np.fromfile(d + "/g%d_out.bin" % i, np.uint32).reshape(H, W, 4), ref[k].view(np.uint32)), k
    assert np.array_equal(np.fromfile(d + "/ao.bin", np.uint16).reshape(H // 2, W // 2), ref["ao"])
    assert np.array_equal(np.fromfile(d + "/out.bin", np.uint8).reshape(H, W, 4), ref["rgba8"])


@pytest.mark.gpu
@pytest.mark.parametrize("cube_levels", [1, 5])
def test_veneer_load_textures(built_lib, oracle, tmp_path, cube_levels):
    """cube_levels = 5: the cube file carries its mip chain (16 .. 1), which LoadTextures binds whole as the reference does
    (CRYCHIC.cpp:1148-1151) -- the frame is then the oracle's with trilinear cube lookups.
    CRYCHIC::LoadTextures through the veneer: the six material textures (with their mip chains) and the sky cube map are read
    from DDS files in a directory laid out like the reference's Textures/, and the frame the veneer then renders -- G-buffer
    sampled anisotropically from those chains, sky and reflections from that cube map -- equals the all-CPU oracle frame fed with
    the oracle's own decode of the same files."""
    import ctypes as C
    import raster_util
    from test_textures import cube_header, mip_header, oracle_cube, oracle_load_mips
    from crychic_renderer_amd import geometry as g, scene
    exe = build_driver()
    W, H, SD, CD, BC, NL = 160, 120, 256, 16, 2, 1
    d = str(tmp_path)
    tdir = tmp_path / "Textures"
    tdir.mkdir()
    names = ["bricks2.dds", "bricks2_nmap.dds", "tile.dds", "tile_nmap.dds", "white1x1.dds", "default_nmap.dds"]
    procedural = g.procedural_textures(32)
    masks = (0xFF0000, 0xFF00, 0xFF, 0xFF000000)                      # A8R8G8B8: memory order B, G, R, A
    for name, t in zip(names, procedural):
        levels = g.box_mips(t)
        (tdir / name).write_bytes(mip_header(32, 32, len(levels), None, masks) + b"".join(np.ascontiguousarray(l[..., [2, 1, 0, 3]]).tobytes() for l in levels))
    rng = np.random.default_rng(3)
    faces = rng.integers(0, 256, (6, CD, CD, 4), dtype=np.uint8)
    face_chains = [g.box_mips(faces[k])[:cube_levels] for k in range(6)]          # file order: face after face, each with its chain
    (tdir / "snowcube1024.dds").write_bytes(cube_header(CD, cube_levels, None, masks) + b"".join(lv.tobytes() for fc in face_chains for lv in fc))
    np.zeros((6, CD, CD, 4), np.uint8).tofile(d + "/cube.bin")        # what SetCubeMap installs first: LoadTextures must replace it
    r = subprocess.run([exe, d, str(W), str(H), str(SD), str(CD), str(BC), str(NL), "scene", str(tdir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    consts = raster_util.frame_constants(W, H, SD)
    C.memmove(C.addressof(consts.ssao_cb), open(d + "/ssao_cb.bin", "rb").read(), C.sizeof(consts.ssao_cb))
    C.memmove(C.addressof(consts.pass_cb), open(d + "/pass_cb.bin", "rb").read(), C.sizeof(consts.pass_cb))
    cam = scene.default_camera(W, H)
    items, shadow_items = g.cascade_scene_items(cull_camera=cam), g.cascade_scene_items(shadow_layer=True, cull_camera=cam)
    tex = [oracle_load_mips(oracle, str(tdir / n)) for n in names]
    cube = oracle_cube(oracle, str(tdir / "snowcube1024.dds"))
    assert np.array_equal(cube, faces[..., [2, 1, 0, 3]])
    chain_kw = {}
    if cube_levels > 1:
        chain, n = g.cube_mip_chain(cube, cube_levels)          # box-filtering commutes with the channel swizzle: == the file's chain
        assert n == cube_levels and np.array_equal(chain, g.load_dds_cube_mips(str(tdir / "snowcube1024.dds"))[0])
        cube, chain_kw = chain, dict(cube_dim=CD, cube_levels=cube_levels)
    ref = raster_util.oracle_frame(oracle, consts, items, shadow_items, g.reference_materials(), tex, W, H, SD, cube, BC, NL,
                                   built_lib.lib.crychic_pcf_search_radius(SD, 1), **chain_kw)
    for i, k in enumerate(("g0", "g1", "g2")):
        assert np.array_equal(np.fromfile(d + "/g%d_out.bin" % i, np.uint32).reshape(H, W, 4), ref[k].view(np.uint32)), k
    assert np.array_equal(np.fromfile(d + "/out.bin", np.uint8).reshape(H, W, 4), ref["rgba8"])
    # the textures do change the frame: the same scene without them (the previous test) has other albedo
    flat = raster_util.oracle_frame(oracle, consts, items, shadow_items, g.reference_materials(), None, W, H, SD, cube, BC, NL,
                                    built_lib.lib.crychic_pcf_search_radius(SD, 1), **chain_kw)
    assert not np.array_equal(flat["g1"], ref["g1"])


@pytest.mark.gpu
def test_veneer_transposes_world_and_texture_transforms(built_lib, oracle, tmp_path):
    """UpdateInstanceData and UpdateMaterialBuffer store World, TexTransform and MatTransform transposed (CRYCHIC.cpp:546-547, 582).
    The live scene never shows it: its World matrices are symmetric in their 3 x 3 and both texture transforms are identity.  The
    driver's `transforms` mode puts the grid under a World with a rotation (3 . RotationY with cos 0.8, sin 0.6, plus a
    translation) and a non-symmetric TexTransform, and its material under a non-symmetric MatTransform; the oracle gets the same
    scene with the records built here, transposed by hand.  Depth, the normal plane and G0 - G2 are equal bit for bit."""
    import ctypes as C
    import raster_util
    from test_textures import cube_header, mip_header, oracle_cube, oracle_load_mips
    from crychic_renderer_amd import geometry as g, scene
    exe = build_driver()
    W, H, SD, CD, BC, NL = 160, 120, 256, 16, 2, 1
    d = str(tmp_path)
    tdir = tmp_path / "Textures"
    tdir.mkdir()
    names = ["bricks2.dds", "bricks2_nmap.dds", "tile.dds", "tile_nmap.dds", "white1x1.dds", "default_nmap.dds"]
    rng = np.random.default_rng(11)
    masks = (0xFF0000, 0xFF00, 0xFF, 0xFF000000)                      # A8R8G8B8: memory order B, G, R, A
    for name in names:                                                # noise: a wrong texture coordinate shows at every pixel
        levels = g.box_mips(rng.integers(0, 256, (32, 32, 4), dtype=np.uint8))
        (tdir / name).write_bytes(mip_header(32, 32, len(levels), None, masks) + b"".join(np.ascontiguousarray(l[..., [2, 1, 0, 3]]).tobytes() for l in levels))
    faces = rng.integers(0, 256, (6, CD, CD, 4), dtype=np.uint8)
    (tdir / "snowcube1024.dds").write_bytes(cube_header(CD, 1, None, masks) + faces.tobytes())
    np.zeros((6, CD, CD, 4), np.uint8).tofile(d + "/cube.bin")
    r = subprocess.run([exe, d, str(W), str(H), str(SD), str(CD), str(BC), str(NL), "transforms", str(tdir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    consts = raster_util.frame_constants(W, H, SD)
    C.memmove(C.addressof(consts.pass_cb), open(d + "/pass_cb.bin", "rb").read(), C.sizeof(consts.pass_cb))
    # the driver's matrices as DirectXMath writes them (rows of v' = v . M); a record holds the transpose
    world = [[2.4, 0, -1.8, 0], [0, 3, 0, 0], [1.8, 0, 2.4, 0], [0.5, 0.125, -0.25, 1]]
    tex_t = [[2, 0.5, 0, 0], [-0.25, 1.5, 0, 0], [0, 0, 1, 0], [0.125, 0.375, 0, 1]]
    mat_t = [[1.25, -0.5, 0, 0], [0.75, 0.5, 0, 0], [0, 0, 1, 0], [0.25, 0.0625, 0, 1]]
    stored = lambda m: np.array([[m[j][i] for j in range(4)] for i in range(4)], np.float32).reshape(16)
    items = g.cascade_scene_items(cull_camera=scene.default_camera(W, H))
    grid_inst = items[1][2].copy()
    assert len(grid_inst) == 1 and grid_inst[0]["MaterialIndex"] == 3
    grid_inst[0]["World"] = stored(world); grid_inst[0]["TexTransform"] = stored(tex_t)
    assert len(g.frustum_cull(scene.default_camera(W, H), items[1][0], grid_inst)) == 1       # still in view under its new World
    items[1] = (items[1][0], items[1][1], grid_inst)
    mats = g.reference_materials().view(oracle_lib.MATERIAL_DT).copy()
    mats[3]["MatTransform"] = stored(mat_t)
    tex = [oracle_load_mips(oracle, str(tdir / n)) for n in names]
    view, vp = np.array(consts.pass_cb.View, np.float32), np.array(consts.pass_cb.ViewProj, np.float32)
    nd = oracle_lib.rasterize(oracle, 1, view, vp, items, mats, tex, W, H)
    gb = oracle_lib.rasterize(oracle, 2, view, vp, items, mats, tex, W, H)
    grid_px = (gb["depth"] < 0xFFFFFF) & (gb["g1"][..., 3] == mats[3]["Roughness"])
    assert grid_px.mean() > 0.1                                        # the grid fills a good part of the frame
    assert np.array_equal(np.fromfile(d + "/depth_out.bin", np.uint32).reshape(H, W), gb["depth"])
    assert np.array_equal(np.fromfile(d + "/normal_out.bin", np.uint16).reshape(H, W, 4), nd["normal"].view(np.uint16))
    for i, k in enumerate(("g0", "g1", "g2")):
        assert np.array_equal(np.fromfile(d + "/g%d_out.bin" % i, np.uint32).reshape(H, W, 4), gb[k].view(np.uint32)), k
    # each of the three matrices matters: with any one of them left untransposed the oracle renders another image
    for which in ("World", "TexTransform", "MatTransform"):
        inst2, mats2 = grid_inst.copy(), mats.copy()
        if which == "MatTransform":
            mats2[3]["MatTransform"] = np.array(mat_t, np.float32).reshape(16)
        else:
            inst2[0][which] = np.array(world if which == "World" else tex_t, np.float32).reshape(16)
        other = oracle_lib.rasterize(oracle, 2, view, vp, [items[0], (items[1][0], items[1][1], inst2)], mats2, tex, W, H)
        assert not all(np.array_equal(other[k], gb[k]) for k in ("g0", "g1", "g2")), which
