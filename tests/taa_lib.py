"""Builds and loads tests/taa_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_taa, plain C written from the definition in
include/crychic_hip.h with none of the kernel's code; and the corpus of matrices, planes and parameters the host and the device tests
share."""
import ctypes as C
import math
import os

import numpy as np

from post_pass_lib import GUARD, DevicePlanes, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "taa_ref")
SRC, LIB = os.path.join(DIR, "taa_ref.c"), os.path.join(DIR, "libtaaref.so")

RESET, NO_CLAMP = 1, 2                                  # CRYCHIC_TAA_RESET, CRYCHIC_TAA_NO_CLAMP
B_HISTORY, B_FX, B_FY, B_CLAMPED = 1, 2, 4, 8           # the bits of the checker's branch plane
DEFAULT_BLEND = 26
TILE_W, TILE_H, WAVE = 32, 8, 8                         # the kernel's workgroup (kTaaGroupW x kTaaTile) and its 8 x 8 wavefront tile
# 1 x 1, 3 x 2, one below / at / one above the workgroup each way (and the two crossings), the five-frame scene's size, an odd frame
SIZES = ((1, 1), (3, 2), (31, 7), (32, 8), (33, 9), (33, 7), (31, 9), (70, 38), (131, 67))
MOTIONS = ("identical", "subpixel_pan", "large_pan", "dolly", "outside", "behind")


def build():
    return build_checker(SRC, LIB)


class Case:
    """One call: InvViewProj of the frame's own constants, the two unjittered view-projections (16 floats each, stored transposed), the
    (H, W) uint32 depth plane, the (H, W, 4) uint8 frame, the (H, W, 4) uint16 history (None only with RESET), blend and flags."""

    def __init__(self, name, ivp, cur, prev, depth, img, hist, blend=DEFAULT_BLEND, flags=0):
        self.name = name
        self.ivp, self.cur, self.prev = (np.ascontiguousarray(m, np.float32).reshape(16).copy() for m in (ivp, cur, prev))
        self.depth = np.ascontiguousarray(depth, np.uint32)
        self.img = np.ascontiguousarray(img, np.uint8)
        self.hist = None if hist is None else np.ascontiguousarray(hist, np.uint16)
        self.blend, self.flags = int(blend), int(flags)
        self.H, self.W = self.img.shape[:2]
        assert self.depth.shape == (self.H, self.W) and self.img.shape == (self.H, self.W, 4)
        assert self.hist is None or self.hist.shape == (self.H, self.W, 4)
        for a in (self.ivp, self.cur, self.prev, self.depth, self.img) + (() if self.hist is None else (self.hist,)):
            a.setflags(write=False)

    def pass_constants(self, lib):
        """A PassConstants of the product's bindings holding this case's InvViewProj (the rest zero)."""
        pcb = lib.PassConstants()
        pcb.InvViewProj[:] = [float(v) for v in self.ivp]
        return pcb


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.taa_ref.argtypes = [C.c_void_p] * 8 + [C.c_uint32] * 6 + [C.c_void_p]
        _REF.taa_ref.restype = None
    return _REF


def checker(case, row0=0, rows=None, out=None, hist_out=None):
    """(out, history_out, branch): rows [row0, row0 + rows) of the resolved (H, W, 4) uint8 frame and of the (H, W, 4) uint16 history
    written into `out` and `hist_out` -- planes of 0xA5 bytes by default --, and the (H, W) uint8 plane of the branch bits of the rows'
    pixels (0 elsewhere)."""
    H, W = case.H, case.W
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    hist_out = np.full((H, W, 4), GUARD * 257, np.uint16) if hist_out is None else hist_out
    branch = np.zeros((H, W), np.uint8)
    _ref().taa_ref(case.ivp.ctypes.data, case.cur.ctypes.data, case.prev.ctypes.data, case.depth.ctypes.data, case.img.ctypes.data,
                   None if case.hist is None else case.hist.ctypes.data, hist_out.ctypes.data, out.ctypes.data, W, H, row0, rows, case.blend,
                   case.flags, branch.ctypes.data)
    return out, hist_out, branch


# ---- matrices ----------------------------------------------------------------------------------------------------------------------

IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def camera_matrices(W, H, cam=None, jitter=(0.0, 0.0)):
    """(ViewProj, InvViewProj), 16 floats each as the pass constants store them, of crychic_update_main_pass_cb_jittered for the
    reference camera (or `cam`) on a W x H frame."""
    from crychic_renderer_amd import _lib, scene
    cam = cam or scene.default_camera(W, H)
    st = np.zeros((4, 4, 4), np.float32)
    dirs = np.asarray(scene.BASE_LIGHT_DIRS, np.float32)
    pcb = _lib.PassConstants()
    _lib.check(_lib.lib.crychic_update_main_pass_cb_jittered(C.byref(cam), W, H, st.ctypes.data, dirs.ctypes.data, jitter[0], jitter[1], C.byref(pcb)))
    return np.array(pcb.ViewProj[:], np.float32), np.array(pcb.InvViewProj[:], np.float32)


def moved_camera(W, H, dx=0.0, dy=0.0, dz=0.0, yaw=0.0, pitch=0.0):
    """The reference camera moved by (dx, dy, dz) and turned by yaw about +y, then pitch about its right axis."""
    from crychic_renderer_amd import scene
    cam = scene.default_camera(W, H)
    cam.pos[:] = (cam.pos[0] + dx, cam.pos[1] + dy, cam.pos[2] + dz)
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    cam.look[:] = (sy * cp, sp, cy * cp)
    cam.up[:] = (-sy * sp, cp, -cy * sp)
    return cam


def motion_matrices(motion, W, H, jitter=(0.25, -0.375)):
    """(InvViewProj of the jittered current frame, unjittered current ViewProj, previous ViewProj) of a named motion."""
    cur, _ = camera_matrices(W, H)
    _, ivp = camera_matrices(W, H, jitter=jitter)
    prev_cam = {
        "identical": None,
        "subpixel_pan": moved_camera(W, H, yaw=0.3 / W),                 # about a third of a pixel at the frame's centre
        "large_pan": moved_camera(W, H, yaw=0.6),                        # more than the 32-pixel tile at the widest frames
        "dolly": moved_camera(W, H, dz=-1.5),                            # velocity varies with depth
        "outside": moved_camera(W, H, yaw=-0.4, pitch=0.25),             # part of the frame outside the history
        "behind": moved_camera(W, H, dz=20.0),                           # the near part of the frame lies behind the previous camera
    }[motion]
    prev = cur if prev_cam is None else camera_matrices(W, H, cam=prev_cam)[0]
    return ivp, cur, prev


def shear_matrices(sx, sy):
    """Synthetic matrices: identity InvViewProj and curViewProj, so that P = (nx, ny, d); a prevViewProj whose x gains sx * d and whose
    y gains sy * d.  A texel of depth 0 has a velocity of exactly 0, one of depth 1 a history sx * W / 2 texels to the right and
    sy * H / 2 texels up of itself."""
    prev = IDENTITY.copy()
    prev[2], prev[6] = sx, sy
    return IDENTITY.copy(), IDENTITY.copy(), prev


def translate_matrices(k, W):
    """Identity InvViewProj and curViewProj and a prevViewProj that translates NDC x by 2 k / W: the history is taken k texels to the
    right (k < 0: to the left) with fx == 0 (W a power of two)."""
    prev = IDENTITY.copy()
    prev[3] = 2.0 * k / W
    return IDENTITY.copy(), IDENTITY.copy(), prev


# ---- planes ------------------------------------------------------------------------------------------------------------------------

def make_depth(kind, W, H, rng):
    if kind == "ones":
        return np.full((H, W), 0xFFFFFF, np.uint32)
    if kind == "ramp":      # the far tenth of the depth range, nearer towards the bottom row, a random top byte
        d = (0xFFFFFF - (np.arange(H)[:, None] * 1600000 // max(H, 1) + np.arange(W)[None, :] * 977)).astype(np.uint32)
        return d | (rng.integers(0, 256, (H, W), dtype=np.uint32) << 24)
    return rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)                # 24 random bits and a random top byte


def make_history(kind, img, rng):
    if kind == "random":    # any uint16, values above 65280 included
        return rng.integers(0, 1 << 16, img.shape, dtype=np.uint16)
    near = img.astype(np.int64) * 256 + rng.integers(-300, 301, img.shape)  # close to the frame: mostly inside the neighbourhood's range
    return np.clip(near, 0, 65535).astype(np.uint16)


def vote_case(name, W, H, sx, sy, one_lane, rng):
    """A depth plane in which exactly one texel of every wavefront's 8 x 8 footprint differs: `one_lane` puts depth 1 into that texel
    and 0 into the rest, otherwise the other way round.  Under shear_matrices a texel of depth 0 stays in place (fx == fy == 0)."""
    d = np.zeros((H, W), np.uint32) if one_lane else np.full((H, W), 0xFFFFFF, np.uint32)
    d[5::WAVE, 3::WAVE] = 0xFFFFFF if one_lane else 0
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    ivp, cur, prev = shear_matrices(sx, sy)
    return Case(name, ivp, cur, prev, d, img, make_history("random", img, rng))


_CORPUS = {}


def corpus():
    """[Case]: built once and read-only.  Every size of SIZES under every motion of MOTIONS, with depth kinds, history kinds, blends and
    flags rotated through them; the vote planes; RESET frames with and without a history plane."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    rng = np.random.default_rng(24)
    cases = []
    blends = (DEFAULT_BLEND, 1, 256, 128, 255)
    v = 0
    for W, H in SIZES:
        for motion in MOTIONS:
            dk = ("random", "ramp", "ones")[v % 3]
            hk = ("random", "near")[(v // 3) % 2]
            blend = blends[v % 5]
            flags = NO_CLAMP if v % 7 == 3 else 0
            ivp, cur, prev = motion_matrices(motion, W, H)
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            cases.append(Case("%dx%d_%s_%s_%s_b%d_f%d" % (W, H, motion, dk, hk, blend, flags), ivp, cur, prev, make_depth(dk, W, H, rng), img,
                              make_history(hk, img, rng), blend, flags))
            v += 1
    # a smooth frame over a history close to it: the clamp mostly leaves the history alone
    W, H = 70, 38
    smooth = np.zeros((H, W, 4), np.uint8)
    smooth[..., 0] = (np.arange(W)[None, :] * 3) & 255
    smooth[..., 1] = (np.arange(H)[:, None] * 5) & 255
    smooth[..., 2] = 90
    smooth[..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for motion in ("identical", "subpixel_pan", "dolly"):
        ivp, cur, prev = motion_matrices(motion, W, H)
        cases.append(Case("smooth_%s" % motion, ivp, cur, prev, make_depth("ramp", W, H, rng), smooth, make_history("near", smooth, rng)))
    # the votes: 64 x 16 is 8 x 2 wavefronts; a shear of half a texel, and one that leaves the frame
    for axis, (sx, sy) in (("fx", (1.0 / 64.0, 0.0)), ("fy", (0.0, 1.0 / 16.0)), ("hist", (8.0, 0.0))):
        for one in (True, False):
            cases.append(vote_case("vote_%s_%s" % (axis, "one_lane" if one else "all_but_one"), 64, 16, sx, sy, one, rng))
    ivp, cur, prev = motion_matrices("dolly", 33, 9)
    img = rng.integers(0, 256, (9, 33, 4), dtype=np.uint8)
    d = make_depth("random", 33, 9, rng)
    cases.append(Case("reset_with_history", ivp, cur, prev, d, img, make_history("random", img, rng), flags=RESET))
    cases.append(Case("reset_null_history", ivp, cur, prev, d, img, None, flags=RESET | NO_CLAMP))
    _CORPUS["cases"] = cases
    return cases


_EXPECTED = {}


def expected(case):
    """The checker's whole-frame (out, history_out, branch) of a corpus case; computed once, read-only."""
    if case.name not in _EXPECTED:
        r = checker(case)
        for a in r:
            a.setflags(write=False)
        _EXPECTED[case.name] = r
    return _EXPECTED[case.name]


def wave_counts(branch, bit):
    """For every whole 8 x 8 wavefront footprint of the plane: the number of its lanes whose branch byte has `bit`."""
    H, W = branch.shape
    b = ((branch[:H - H % WAVE, :W - W % WAVE] & bit) != 0).astype(np.int64)
    return b.reshape(H // WAVE, WAVE, W // WAVE, WAVE).sum(axis=(1, 3)).reshape(-1)


# ---- the still reference scene under jitter (the convergence test and tests/taa_quality.py) -----------------------------------------

def jitter(index):
    from crychic_renderer_amd import _lib
    jx, jy = C.c_float(), C.c_float()
    _lib.check(_lib.lib.crychic_taa_jitter(index, C.byref(jx), C.byref(jy)))
    return jx.value, jy.value


class StillScene:
    """The reference scene lit by the CPU oracle (blurCount 3, 3 lights, sky) under any jitter: the cascades, the cube map and the
    random vectors are built once, the camera planes per jitter."""

    def __init__(self, W, H, shadow_dim=512, cube_dim=64):
        import oracle_lib
        from crychic_renderer_amd import scene
        self.W, self.H, self.shadow_dim = W, H, shadow_dim
        self.orc = oracle_lib.load()
        self.base = scene.make_scene(W, H, shadow_dim=shadow_dim, cube_dim=cube_dim, device="cpu")
        self.cur = np.array(self.base["consts"].pass_cb.ViewProj[:], np.float32)

    def frame(self, jit=(0.0, 0.0)):
        """(lit (H, W, 4) uint8 frame, (H, W) uint32 depth plane, InvViewProj of the jittered constants)."""
        import oracle_lib
        import scene_util
        from crychic_renderer_amd import lib, scene
        consts = scene.Constants(self.W, self.H, self.shadow_dim, jitter=jit)
        planes = dict(self.base, **scene._camera_planes(consts, "cpu"))
        p = scene_util.np_planes(planes)
        scb = oracle_lib.as_oracle_cb(consts.ssao_cb, oracle_lib.OrSsaoConstants)
        pcb = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
        ao = self.orc.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)
        lit = self.orc.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], ao, p["shadow"], p["cube"], 3,
                                      lib.crychic_pcf_search_radius(self.shadow_dim, 1), sky=True)
        return np.ascontiguousarray(lit), np.ascontiguousarray(p["depth"]), np.array(consts.pass_cb.InvViewProj[:], np.float32)

    def resolve(self, frames, blend=DEFAULT_BLEND):
        """The checker's resolved frame after `frames` jittered frames of the still camera, the first a RESET frame."""
        hist, out = None, None
        for k in range(frames):
            lit, depth, ivp = self.frame(jitter(k))
            out, hist, _ = checker(Case("still%d" % k, ivp, self.cur, self.cur, depth, lit, hist, blend, RESET if hist is None else 0))
        return out


def box_filter(big, f):
    """The (H f, W f, 4) frame averaged over f x f blocks, rounded per channel."""
    H, W = big.shape[0] // f, big.shape[1] // f
    s = big.astype(np.int64).reshape(H, f, W, f, 4).sum(axis=(1, 3))
    return ((s + f * f // 2) // (f * f)).astype(np.int32)


# ---- the device (GPU tier) ------------------------------------------------------------------------------------------------------------

def run_device(dev, case, row0=0, rows=None, misalign=0):
    """crychic_taa on guarded device copies of the case's planes, the frame planes `misalign` bytes and the history planes
    `misalign & 8` bytes past a 256-byte boundary: (out, history_out) as numpy, the guards and the inputs checked.  dev = (the
    product's _lib module, a Context, torch)."""
    lib, ctx, torch = dev
    H, W = case.H, case.W
    planes = DevicePlanes(dev)
    src = planes.upload("input", case.img, misalign)
    depth = planes.upload("depth", case.depth, misalign)
    out = planes.blank("out", case.img.shape, np.uint8, misalign)
    hout = planes.blank("history out", (H, W, 4), np.uint16, misalign & 8)
    hin = None if case.hist is None else planes.upload("history in", case.hist, misalign & 8)
    pcb = case.pass_constants(lib)
    p = lib.TaaParams.default(blend=case.blend, flags=case.flags)
    cur, prev = (C.c_float * 16)(*case.cur), (C.c_float * 16)(*case.prev)
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_taa(ctx.handle, C.byref(pcb), cur, prev, C.c_void_p(depth.data_ptr()), C.c_void_p(src.data_ptr()),
                                  None if hin is None else C.c_void_p(hin.data_ptr()), C.c_void_p(hout.data_ptr()), C.c_void_p(out.data_ptr()), W, H,
                                  row0, H - row0 if rows is None else rows, C.byref(p), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return out.cpu().numpy().reshape(H, W, 4), hout.cpu().numpy().view(np.uint16).reshape(H, W, 4)
