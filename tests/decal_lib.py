"""Builds and loads tests/decal_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_apply_decals, plain C written from the
definition in include/crychic_hip.h with none of the kernel's code; and the corpus of frames, decals and textures the host and the
device tests share."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "decal_ref")
SRC, LIB = os.path.join(DIR, "decal_ref.c"), os.path.join(DIR, "libdecalref.so")
GOLD = os.path.join(ROOT, "tests", "golden", "frame_64x64.npz")

COUNTERS = ("uncovered", "outside_bounds", "outside_box", "fade_zero", "fade_partial", "fade_one", "a_not_positive", "one_level", "lod_low",
            "lod_interior", "lod_high", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "store_albedo", "store_roughness",
            "store_metalness", "store_normal", "normal_no_map", "bad_texture", "nonfinite_position")
ALBEDO, ROUGHNESS, METALNESS, NORMAL = 1, 2, 4, 8
NO_TEXTURE = 0xFFFFFFFF
MIXES = {"f32": 0, "mixed": 0x6000, "f16": 0x7000}        # CRYCHIC_GBUFFER_G*_F16 bits: G1 and G2 half, all three half
SIZES = ((1, 1), (3, 5), (63, 4), (64, 4), (65, 7), (130, 9))

DECAL = np.dtype([("invWorld", "f4", 12), ("boundsMin", "f4", 3), ("boundsMax", "f4", 3), ("tangentW", "f4", 3), ("bitangentW", "f4", 3),
                  ("normalW", "f4", 3), ("tint", "f4", 3), ("opacity", "f4"), ("roughness", "f4"), ("metalness", "f4"), ("fadeScale", "f4"),
                  ("fadeBias", "f4"), ("texelsPerUnit", "f4"), ("texture", "u4"), ("normalTexture", "u4"), ("flags", "u4"), ("reserved", "u4")])
assert DECAL.itemsize == 160


class RefTexture(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("mipLevels", C.c_uint32)]


def build():
    return build_checker(SRC, LIB)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.decal_ref.argtypes = [C.c_void_p, C.c_float] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 2
        _REF.decal_ref.restype = None
        _REF.decal_ref_f2h.argtypes, _REF.decal_ref_f2h.restype = [C.c_float], C.c_uint16
        _REF.decal_ref_h2f.argtypes, _REF.decal_ref_h2f.restype = [C.c_uint16], C.c_float
    return _REF


# ---- decals and textures ---------------------------------------------------------------------------------------------------------

def box_world(center, half, yaw=0.0, rot=None):
    """The unit cube -> world matrix (16 floats, the layout of crychic_instance_data.World) of a box with the given centre and half
    extents, turned by `yaw` radians about +y or by the 3 x 3 rotation `rot`."""
    R = np.eye(3) if rot is None else np.asarray(rot, np.float64)
    if rot is None and yaw:
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    M = np.eye(4)
    M[:3, :3] = R * (2.0 * np.asarray(half, np.float64))[None, :]
    M[:3, 3] = center
    return M.astype(np.float32).reshape(16)


def floor_world(center, half, yaw=0.0):
    """A box that looks DOWN (its +z is world +y, so it lands on surfaces whose normals point up): local x = world x, local y = world
    z, both turned by `yaw` about +y; `half` is given in world x, y, z."""
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, s, 0], [0, 0, 1], [-s, c, 0]], np.float64)      # columns: the images of local x, y, z
    return box_world(center, (half[0], half[2], half[1]), rot=R)


def wall_world(center, half):
    """A box whose +z is world -z (it lands on faces whose normals point to -z): local x = world -x, local y = world y."""
    R = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float64)
    return box_world(center, half, rot=R)


def decal_from_box(world, tex_size, cos_start=1.0, cos_end=1.0, **fields):
    """One DECAL record from the library's crychic_decal_from_box, with `fields` set afterwards."""
    from crychic_renderer_amd import _lib
    d = _lib.Decal()
    w = (C.c_float * 16)(*[float(x) for x in world])
    _lib.check(_lib.lib.crychic_decal_from_box(w, int(tex_size[0]), int(tex_size[1]), cos_start, cos_end, C.byref(d)))
    rec = np.frombuffer(bytes(d), DECAL).copy()
    for k, v in fields.items():
        rec[k] = v
    return rec


def decals_array(records):
    return np.concatenate(records) if len(records) else np.zeros(0, DECAL)


def level_sizes(w, h, levels):
    return [(max(1, w >> k), max(1, h >> k)) for k in range(max(levels, 1))]


def random_texture(rng, w, h, levels, alpha=None):
    """(flat uint8 chain, w, h, levels): random bytes in every level (the levels need not be one another's filtered images for the
    arithmetic to be checked); a tenth of the alphas 0 and a tenth 255 unless `alpha` fixes them."""
    n = sum(a * b for a, b in level_sizes(w, h, levels))
    t = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    if alpha is None:
        r = rng.random(n)
        t[r < 0.1, 3] = 0
        t[r > 0.9, 3] = 255
    else:
        t[:, 3] = alpha
    return (np.ascontiguousarray(t.reshape(-1)), w, h, levels)


def solid_texture(rgba, w=1, h=1):
    return (np.ascontiguousarray(np.tile(np.asarray(rgba, np.uint8), w * h)), w, h, 1)


def ref_textures(textures):
    arr = (RefTexture * max(len(textures), 1))()
    for k, (t, w, h, levels) in enumerate(textures):
        arr[k] = RefTexture(t.ctypes.data, w, h, levels)
    return arr


# ---- frames ----------------------------------------------------------------------------------------------------------------------

class Frame:
    """What the pass reads besides the decals: View and Proj (16 floats each, stored transposed), the (H, W) uint32 depth plane and
    the three (H, W, 4) float32 planes; planes(mix) gives them in a format mix, as (uint8 bytes reshaped (H, W, 16 or 8))."""

    def __init__(self, view, proj, depth, g0, g1, g2):
        self.view = np.ascontiguousarray(view, np.float32).reshape(16).copy()
        self.proj = np.ascontiguousarray(proj, np.float32).reshape(16).copy()
        self.depth = np.ascontiguousarray(depth, np.uint32)
        self.g = [np.ascontiguousarray(p, np.float32) for p in (g0, g1, g2)]
        self.H, self.W = self.depth.shape
        self._planes = {}

    def planes(self, mix):
        """[g0, g1, g2] as read-only uint8 arrays (H, W, 16) or (H, W, 8) in the formats of `mix`."""
        if mix not in self._planes:
            out = []
            for k, p in enumerate(self.g):
                with np.errstate(over="ignore", invalid="ignore"):
                    q = p.astype(np.float16) if MIXES[mix] & (0x1000 << k) else p
                b = np.ascontiguousarray(q).view(np.uint8).reshape(self.H, self.W, -1)
                b.setflags(write=False)
                out.append(b)
            self._planes[mix] = out
        return self._planes[mix]

    def values(self, mix):
        """The planes of `mix` widened to float32: what the pass sees."""
        return [b.view(np.float16).astype(np.float32) if b.shape[2] == 8 else b.view(np.float32) for b in self.planes(mix)]

    def pass_constants(self):
        from crychic_renderer_amd import _lib
        pcb = _lib.PassConstants()
        for k in range(16):
            pcb.View[k], pcb.Proj[k] = float(self.view[k]), float(self.proj[k])
        return pcb


def checker(frame, mix, decals, textures, row0=0, rows=None, planes=None, passed=False):
    """([g0, g1, g2] after the pass over rows [row0, row0 + rows) -- copies of frame.planes(mix), or `planes` modified in place --,
    {counter: count}); with passed=True a third value, the (H, W) uint64 plane of the decals each pixel passes step 2 of."""
    H, W = frame.H, frame.W
    rows = H - row0 if rows is None else rows
    planes = [p.copy() for p in frame.planes(mix)] if planes is None else planes
    decals = np.ascontiguousarray(decals)
    n = np.zeros(len(COUNTERS), np.uint64)
    p2 = np.zeros((H, W), np.uint64) if passed else None
    tex = ref_textures(textures)
    vz = frame.view[8:12].copy()
    _ref().decal_ref(vz.ctypes.data, float(frame.proj[5]), frame.depth.ctypes.data, planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data,
                     MIXES[mix], decals.ctypes.data if len(decals) else None, len(decals), C.addressof(tex), len(textures), W, H, row0, rows,
                     n.ctypes.data, None if p2 is None else p2.ctypes.data)
    counts = dict(zip(COUNTERS, (int(v) for v in n)))
    return (planes, counts, p2) if passed else (planes, counts)


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

_SCENE = {}


def scene_frame():
    """The 128 x 96 synthetic scene (crychic_renderer_amd.scene, on the CPU): its camera, depth plane and G-buffer."""
    if "frame" not in _SCENE:
        from crychic_renderer_amd import scene
        planes = scene.make_scene(128, 96, shadow_dim=64, cube_dim=8, device="cpu")
        f = np.frombuffer(bytes(planes["consts"].pass_cb), np.float32)
        _SCENE["frame"] = Frame(f[0:16], f[32:48], planes["depth"].numpy().view(np.uint32), planes["g0"].numpy(), planes["g1"].numpy(), planes["g2"].numpy())
    return _SCENE["frame"]


def golden_frame():
    g = np.load(GOLD, allow_pickle=False)
    f = np.frombuffer(g["pass_cb"].tobytes(), np.float32)
    return Frame(f[0:16], f[32:48], g["depth"], g["g0"], g["g1"], g["g2"])


# the issue's five boxes on the scene frame: (name, world matrix, pixels inside, tiles with a pixel inside)
def scene_boxes():
    return [("floor", floor_world((2.5, 0.0, -7.5), (1.5, 0.25, 1.5)), 510, 12),
            ("floor_yaw30", floor_world((2.5, 0.0, -7.5), (1.5, 0.25, 1.5), yaw=-np.pi / 6), 524, 15),
            ("box_face", wall_world((0.0, 0.8, -10.8), (0.6, 0.6, 0.3)), 1054, 24),
            ("lane", floor_world((2.5, 0.0, 10.0), (1.0, 0.25, 12.0)), 30, 5),
            ("everything", floor_world((0.0, 0.0, 0.0), (12.0, 2.0, 12.0)), 5746, 96)]


def camera_frame(W, H, rng, n_bad=3):
    """A random frame under the reference camera: positions in [-4, 4]^3 with NaN and +-inf sprinkled in, random normals with zero
    vectors, a quarter of the depth words 0xFFFFFF, garbage in the top byte."""
    sc = scene_frame()
    g0 = rng.uniform(-4, 4, (H, W, 4)).astype(np.float32)
    g0[..., 3] = rng.random((H, W), np.float32)
    g1 = rng.random((H, W, 4), np.float32)
    g2 = rng.normal(size=(H, W, 4)).astype(np.float32)
    g2[rng.random((H, W)) < 0.05, :3] = 0.0
    bad = rng.random((H, W))
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        m = (bad > 0.02 * k) & (bad < 0.02 * (k + 1))
        g0[m, rng.integers(0, 3)] = v
    if W * H >= n_bad:
        flat = g0.reshape(-1, 4)
        for k, v in enumerate((np.nan, np.inf, -np.inf)[:n_bad]):
            flat[(k * 7) % (W * H), k % 3] = v
    depth = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
    depth[rng.random((H, W)) < 0.25] |= 0xFFFFFF
    proj = sc.proj.copy()
    proj[5] = proj[5] * 0.02            # a pixel a fiftieth as fine: the lods of positions 4 .. 20 units away spread over the chains
    return Frame(sc.view, proj, depth, g0, g1, g2)


def random_rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


TEXTURE_SHAPES = ((1, 1, 1), (2, 2, 1), (5, 3, 3), (16, 16, 5), (16, 16, 1), (4, 8, 4))


def random_case(rng, W, H, n, mix):
    textures = [random_texture(rng, w, h, L) for (w, h, L) in TEXTURE_SHAPES]
    frame = camera_frame(W, H, rng)
    recs = []
    for d in range(n):
        big = rng.random() < 0.5
        half = rng.uniform(2.0, 6.0, 3) if big else rng.uniform(0.3, 2.0, 3)
        world = box_world(rng.uniform(-3, 3, 3), half, rot=random_rotation(rng))
        ti = int(rng.integers(0, len(textures)))
        start, end = ((1.0, 1.0), (0.8, -0.3), (0.2, -0.9))[int(rng.integers(0, 3))]
        rec = decal_from_box(world, textures[ti][1:3], start, end, texture=ti, flags=int(rng.integers(1, 16)),
                             tint=rng.random(3), opacity=rng.choice([1.0, 0.6, 0.0], p=[0.5, 0.4, 0.1]), roughness=rng.random(),
                             metalness=rng.random())
        r = rng.random()
        rec["normalTexture"] = NO_TEXTURE if r < 0.3 else int(rng.integers(0, len(textures)))
        if rng.random() < 0.1:
            rec["texture"] = len(textures) + int(rng.integers(0, 3))                   # out of range: the decal changes nothing
        if rng.random() < 0.1:
            rec["texelsPerUnit"] *= rng.choice([1e-3, 1e3])                            # the lod clamps low / high
        recs.append(rec)
    return frame, decals_array(recs), textures, mix


# ---- the two texture known answers, shared by the host and the device tests ------------------------------------------------------

def inside_box(frame, rec, margin):
    """The covered pixels whose |q| stays below 0.5 + margin in float64: clear of the faces for a negative margin."""
    P = frame.g[0][..., :3].astype(np.float64)
    iw = rec["invWorld"][0].astype(np.float64)
    q = np.stack([np.abs(P @ iw[4 * c:4 * c + 3] + iw[4 * c + 3]) for c in range(3)], -1)
    return ((frame.depth & 0xFFFFFF) < 0xFFFFFF) & (q < 0.5 + margin).all(-1)


def grey_levels_case():
    """(frame, decal, textures): the scene with albedo 0 (lerpf(0, t, 1) is t exactly) under the lane decal (view depths 13 .. 36) with
    a 16 x 16 chain whose level k is grey 16 k, opaque; a pixel is 0.11 .. 0.31 units wide there: lod 0.8 .. 2.3 of the five levels."""
    sc = scene_frame()
    chain = np.concatenate([np.tile(np.array([16 * k, 16 * k, 16 * k, 255], np.uint8), w * h) for k, (w, h) in enumerate(level_sizes(16, 16, 5))])
    rec = decal_from_box(floor_world((2.5, 0.0, 10.0), (1.0, 0.25, 12.0)), (16, 16), texelsPerUnit=16.0)
    return Frame(sc.view, sc.proj, sc.depth, sc.g[0], np.zeros_like(sc.g[1]), sc.g[2]), rec, [(chain, 16, 16, 5)]


def assert_grey_does_not_fall(frame, rec, g1):
    """`g1`: the G1 plane (bytes) after grey_levels_case.  Sorted by view depth, the grey inside the decal does not fall, rises overall
    and stays between levels 0 and 3."""
    inside = inside_box(frame, rec, -1e-4)
    assert inside.sum() >= 25
    vz = frame.view[8:12].astype(np.float64)
    depth = frame.g[0][..., :3].astype(np.float64) @ vz[:3] + vz[3]
    assert depth[inside].min() > 12.5 and depth[inside].max() < 36.5
    grey = g1.view(np.float32)[inside][np.argsort(depth[inside], kind="stable"), 0]
    assert (np.diff(grey) >= 0).all() and grey[-1] > grey[0] + 0.05 and 0.0 < grey[0] and grey[-1] < 48.0 / 255.0


def red_blue_case():
    """(frame, decal, textures): two pixels at the unit cube's u = 0 and u = 1 under a 2 x 1 texture, left texel red, right blue:
    CLAMP gives pure red and pure blue (assert_red_blue), WRAP would mix them."""
    sc = scene_frame()
    flat = Frame(sc.view, sc.proj, np.zeros((1, 2), np.uint32), np.array([[[-0.5, 0, 0, 0], [0.5, 0, 0, 0]]], np.float32),
                 np.zeros((1, 2, 4), np.float32), np.array([[[0, 0, 1, 0]] * 2], np.float32))
    return flat, decal_from_box(box_world((0, 0, 0), (0.5, 0.5, 0.5)), (2, 1)), [(np.array([255, 0, 0, 255, 0, 0, 255, 255], np.uint8), 2, 1, 1)]


def assert_red_blue(g1):
    g1 = g1.view(np.float32)
    assert np.array_equal(g1[0, 0, :3], [1, 0, 0]) and np.array_equal(g1[0, 1, :3], [0, 0, 1])


_CORPUS = {}


def case_names():
    """The names of corpus(), in its order, without building it (for test ids at collection time)."""
    mixes = list(MIXES)
    names = ["scene_" + n for n in ("floor", "floor_yaw30", "box_face", "lane", "everything")] + ["scene_all_" + m for m in mixes] + ["golden64"]
    k = 0
    for (W, H) in SIZES:
        for n in (0, 1, 63, 64):
            names.append("%dx%d_n%d_%s" % (W, H, n, mixes[k % 3]))
            k += 1
    return names


def corpus():
    """[(name, Frame, decals, textures, mix)]: built once and read-only.  The scene frame under each of the issue's boxes and under
    all of them with normal maps and fades, the golden frame, and every size of SIZES under decal counts 0, 1, 63, 64 and the three
    mixes."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    rng = np.random.default_rng(22)
    cases = []
    sc, gold = scene_frame(), golden_frame()
    tex = [random_texture(rng, 16, 16, 5, alpha=255), random_texture(rng, 5, 3, 3), random_texture(rng, 2, 2, 1)]
    mixes = list(MIXES)
    for k, (name, world, _, _) in enumerate(scene_boxes()):
        rec = decal_from_box(world, (16, 16), 0.5, -0.5, texture=0, normalTexture=1, flags=15, roughness=0.1, metalness=0.9, tint=(0.9, 0.5, 0.2))
        cases.append(("scene_" + name, sc, decals_array([rec]), tex, mixes[k % 3]))
    stack = [decal_from_box(w, (5, 3), 0.5, -0.5, texture=1 + (k & 1), normalTexture=k % 3, flags=1 + 2 * k, opacity=0.7) for k, (_, w, _, _) in enumerate(scene_boxes())]
    flipped = decal_from_box(box_world((0.0, 0.0, 0.0), (12.0, 12.0, 2.0), rot=np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])),      # its +z is world -y
                             (16, 16), 0.5, -0.5, texture=0, flags=3)
    for mix in mixes:
        cases.append(("scene_all_" + mix, sc, decals_array(stack + [flipped]), tex, mix))
    cases.append(("golden64", gold, decals_array(stack), tex, "f32"))
    k = 0
    for (W, H) in SIZES:
        for n in (0, 1, 63, 64):
            cases.append(("%dx%d_n%d_%s" % (W, H, n, mixes[k % 3]),) + random_case(rng, W, H, n, mixes[k % 3]))
            k += 1
    for case in cases:
        f = case[1]
        for arr in [f.view, f.proj, f.depth, case[2]] + f.g + [t[0] for t in case[3]]:
            arr.setflags(write=False)
    assert [c[0] for c in cases] == case_names()
    _CORPUS["cases"] = cases
    return cases


def case(name):
    return {c[0]: c for c in corpus()}[name]


_EXPECTED = {}


def expected(name):
    """The checker's planes, counters and step-2 plane for corpus case `name`; computed once, read-only."""
    if name not in _EXPECTED:
        _, frame, decals, textures, mix = case(name)
        planes, n, p2 = checker(frame, mix, decals, textures, passed=True)
        for p in planes:
            p.setflags(write=False)
        _EXPECTED[name] = (planes, n, p2)
    return _EXPECTED[name]


def total_counters():
    tot = dict.fromkeys(COUNTERS, 0)
    for c in corpus():
        for k, v in expected(c[0])[1].items():
            tot[k] += v
    return tot
