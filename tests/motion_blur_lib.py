"""Builds and loads tests/motion_blur_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_motion_blur, plain C written from the
definition in include/crychic_hip.h with none of the kernels' code; and the corpus of matrices, planes and parameters the host and the
device tests share."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, DevicePlanes, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share
import taa_lib
from taa_lib import IDENTITY, camera_matrices, moved_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "motion_blur_ref")
SRC, LIB = os.path.join(DIR, "motion_blur_ref.c"), os.path.join(DIR, "libmotionblurref.so")

B_STILL, B_CLAMPED, B_INVALID, B_FRONT, B_BACK = 1, 2, 4, 8, 16       # the bits of the checker's branch plane
BRANCHES = {"still": B_STILL, "clamped": B_CLAMPED, "invalid": B_INVALID, "front": B_FRONT, "back": B_BACK}
TILE = 16
DEFAULT_SHUTTER, DEFAULT_SAMPLES, DEFAULT_RADIUS = 128, 8, 16
# 1 x 1, one pixel past a tile in a single row, exactly one tile, partial tiles on both edges twice (3 x 4 and 5 x 3 tiles)
SIZES = ((1, 1), (17, 1), (16, 16), (33, 49), (70, 38))
CAMERAS = ("still", "strafe", "yaw", "dolly", "clamp", "behind", "nan", "inf")
SAMPLES = (2, 4, 8, 16, 32)
RADII = (1, 16, 32)
SHUTTERS = (0, 1, 128, 256)


def build():
    return build_checker(SRC, LIB)


def tiles(n):
    return (n + TILE - 1) // TILE


def tile_offset(W, H):
    return W * H * 8


def workspace_bytes(W, H):
    return W * H * 8 + tiles(W) * tiles(H) * 4


class Case:
    """One call: InvViewProj of the frame's constants, the two unjittered view-projections (16 floats each, stored transposed), the
    (H, W) uint32 depth plane, the (H, W, 4) uint8 frame and the three parameters."""

    def __init__(self, name, ivp, cur, prev, depth, img, shutter=DEFAULT_SHUTTER, samples=DEFAULT_SAMPLES, radius=DEFAULT_RADIUS):
        self.name = name
        self.ivp, self.cur, self.prev = (np.ascontiguousarray(m, np.float32).reshape(16).copy() for m in (ivp, cur, prev))
        self.depth = np.ascontiguousarray(depth, np.uint32)
        self.img = np.ascontiguousarray(img, np.uint8)
        self.shutter, self.samples, self.radius = int(shutter), int(samples), int(radius)
        self.H, self.W = self.img.shape[:2]
        assert self.depth.shape == (self.H, self.W) and self.img.shape == (self.H, self.W, 4)
        for a in (self.ivp, self.cur, self.prev, self.depth, self.img):
            a.setflags(write=False)

    def pass_constants(self, lib):
        """A PassConstants of the product's bindings holding this case's InvViewProj (the rest zero)."""
        pcb = lib.PassConstants()
        pcb.InvViewProj[:] = [float(v) for v in self.ivp]
        return pcb

    def params(self, lib):
        return lib.MotionBlurParams.default(shutter=self.shutter, samples=self.samples, maxRadius=self.radius)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.motion_blur_ref_velocity.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_void_p] * 2
        _REF.motion_blur_ref_velocity.restype = None
        _REF.motion_blur_ref_gather.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 5 + [C.c_void_p] * 2
        _REF.motion_blur_ref_gather.restype = None
    return _REF


def checker_velocity(case):
    """(workspace, branch): the workspace_bytes(W, H) bytes of steps A and A' as a uint8 array, and the (H, W) uint8 branch plane with
    the clamped and invalid bits."""
    H, W = case.H, case.W
    ws = np.full(workspace_bytes(W, H), GUARD, np.uint8)
    branch = np.zeros((H, W), np.uint8)
    _ref().motion_blur_ref_velocity(case.ivp.ctypes.data, case.cur.ctypes.data, case.prev.ctypes.data, case.depth.ctypes.data, W, H, case.shutter,
                                    case.radius, ws.ctypes.data, branch.ctypes.data)
    return ws, branch


def checker_gather(case, ws, row0=0, rows=None, out=None, branch=None, img=None):
    """Rows [row0, row0 + rows) of step B from the workspace `ws` into `out` (a plane of 0xA5 bytes by default); the still, front and
    back bits of the rows' pixels are ORed into `branch`.  `img` replaces the case's frame."""
    H, W = case.H, case.W
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    img = case.img if img is None else np.ascontiguousarray(img, np.uint8)
    _ref().motion_blur_ref_gather(img.ctypes.data, out.ctypes.data, W, H, row0, rows, case.samples, ws.ctypes.data,
                                  None if branch is None else branch.ctypes.data)
    return out


_EXPECTED = {}


def expected(case):
    """The checker's whole-frame (workspace, out, branch) of a corpus case; computed once, read-only."""
    if case.name not in _EXPECTED:
        ws, branch = checker_velocity(case)
        out = checker_gather(case, ws, branch=branch)
        for a in (ws, out, branch):
            a.setflags(write=False)
        _EXPECTED[case.name] = (ws, out, branch)
    return _EXPECTED[case.name]


def velocity_words(ws, W, H):
    """The (H, W) uint32 plane of velocity words, the (H, W) plane of depth fields and the (tilesY, tilesX) tile plane of a workspace."""
    v = ws[:W * H * 8].view(np.uint32).reshape(H, W, 2)
    return v[..., 0], v[..., 1], ws[W * H * 8:workspace_bytes(W, H)].view(np.uint32).reshape(tiles(H), tiles(W))


def word(qx, qy):
    return (qx & 0xFFFF) | ((qy & 0xFFFF) << 16)


# ---- matrices ----------------------------------------------------------------------------------------------------------------------

def camera_motion(camera, W, H):
    """(InvViewProj, current ViewProj, previous ViewProj) of a named camera move on a W x H frame."""
    cur, ivp = camera_matrices(W, H)
    if camera in ("still", "nan", "inf"):
        prev = cur.copy()
        if camera == "nan":         # the previous w column: every b[3] is NaN
            prev[12] = np.float32("nan")
        if camera == "inf":         # the current x column: a[0] is infinite, and inf - inf where it meets itself
            cur = cur.copy()
            cur[0] = np.float32("inf")
        return ivp, cur, prev
    prev_cam = {
        "strafe": moved_camera(W, H, dx=0.35),                            # velocity falls with depth
        "yaw": moved_camera(W, H, yaw=0.12),                              # nearly uniform, several pixels
        "dolly": moved_camera(W, H, dz=-1.5),                             # radial, zero at the centre
        "clamp": moved_camera(W, H, yaw=0.9, pitch=-0.3),                 # further than any R
        "behind": moved_camera(W, H, dz=20.0),                            # the near part of the frame lies behind the previous camera
    }[camera]
    return ivp, cur, camera_matrices(W, H, cam=prev_cam)[0]


def translate_matrices(kx, ky, W, H):
    """Identity InvViewProj and curViewProj and a prevViewProj that translates NDC by (2 kx / W, -2 ky / H): every pixel's velocity is
    (-kx, -ky) pixels whatever its depth, exactly so for W and H powers of two."""
    prev = IDENTITY.copy()
    prev[3], prev[7] = 2.0 * kx / W, -2.0 * ky / H
    return IDENTITY.copy(), IDENTITY.copy(), prev


def shear_matrices(sx, sy):
    """As taa_lib.shear_matrices: P = (nx, ny, d); a texel of depth 0 stands still, one of depth 1 moves by (-sx W / 2, sy H / 2) pixels."""
    return taa_lib.shear_matrices(sx, sy)


def make_depth(kind, W, H, rng):
    if kind == "layers":    # two depths in vertical bands of 5 pixels, the nearer one every other band
        d = np.where((np.arange(W)[None, :] // 5) % 2 == 0, 0x400000, 0xFFFFFF).astype(np.uint32) + np.zeros((H, 1), np.uint32)
        return d | (rng.integers(0, 256, (H, W), dtype=np.uint32) << 24)
    return taa_lib.make_depth(kind, W, H, rng)


_CORPUS = {}


def corpus():
    """[Case]: built once and read-only.  Every size of SIZES under every camera of CAMERAS with depth kinds and parameters rotated
    through them, so that every N, R and shutter occurs at every size; then synthetic motions: uniform translations, shears over
    layered depth, and the tie of two equal lengths."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    rng = np.random.default_rng(25)
    cases = []
    v = 0
    for W, H in SIZES:
        for camera in CAMERAS:
            dk = ("ramp", "random", "ones", "layers")[v % 4]
            n, r, sh = SAMPLES[v % 5], RADII[v % 3], SHUTTERS[(v + v // 4) % 4]
            ivp, cur, prev = camera_motion(camera, W, H)
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            cases.append(Case("%dx%d_%s_%s_n%d_r%d_s%d" % (W, H, camera, dk, n, r, sh), ivp, cur, prev, make_depth(dk, W, H, rng), img, sh, n, r))
            v += 1
    for W, H in ((33, 49), (70, 38), (64, 32)):
        for k, (kx, ky) in enumerate(((3.0, 0.0), (0.0, -2.5), (-7.25, 4.0), (40.0, 40.0), (0.4, 0.0))):
            ivp, cur, prev = translate_matrices(kx, ky, W, H)
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            cases.append(Case("%dx%d_translate%d_n%d" % (W, H, k, SAMPLES[(k + W) % 5]), ivp, cur, prev, make_depth(("random", "layers")[k % 2], W, H, rng),
                              img, (256, 128)[k % 2], SAMPLES[(k + W) % 5], RADII[1 + k % 2]))
        for k, (sx, sy) in enumerate(((0.5, 0.0), (-0.2, 0.3), (4.0, 1.0))):
            ivp, cur, prev = shear_matrices(sx, sy)
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            cases.append(Case("%dx%d_shear%d" % (W, H, k), ivp, cur, prev, make_depth(("layers", "random", "ramp")[k], W, H, rng), img, 256,
                              SAMPLES[(k + 2) % 5], RADII[(k + 1) % 3]))
    _CORPUS["cases"] = cases
    return cases


# ---- the device (GPU tier) ------------------------------------------------------------------------------------------------------------

def run_device(dev, case, row0=0, rows=None, misalign=0, entry="both", ws_host=None):
    """crychic_motion_blur on guarded device copies of the case's planes, the frame planes `misalign` bytes and the workspace
    `misalign & 8` bytes past a 256-byte boundary: (workspace bytes, out) as numpy, the guards and the inputs checked.  entry: "both"
    (crychic_motion_blur, whole frame), "split" (the velocity entry, then the gather entry over the row range) or "gather" (the gather
    entry alone over the workspace bytes `ws_host`).  dev = (the product's _lib module, a Context, torch)."""
    lib, ctx, torch = dev
    H, W = case.H, case.W
    rows = H - row0 if rows is None else rows
    need = workspace_bytes(W, H)
    planes = DevicePlanes(dev)
    src = planes.upload("input", case.img, misalign)
    depth = planes.upload("depth", case.depth, misalign)
    out = planes.blank("out", case.img.shape, np.uint8, misalign)
    ws = planes.upload("workspace", np.full(need, GUARD, np.uint8) if ws_host is None else ws_host, misalign & 8, writable=True)
    pcb = case.pass_constants(lib)
    p = case.params(lib)
    cur, prev = (C.c_float * 16)(*case.cur), (C.c_float * 16)(*case.prev)
    s = torch.cuda.current_stream(ctx.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(s.cuda_stream)
    if entry == "both":
        assert row0 == 0 and rows == H
        lib.check(lib.lib.crychic_motion_blur(ctx.handle, C.byref(pcb), cur, prev, ptr(depth), ptr(src), ptr(out), W, H, C.byref(p), ptr(ws), need, st))
    else:
        if entry == "split":
            lib.check(lib.lib.crychic_motion_blur_velocity(ctx.handle, C.byref(pcb), cur, prev, ptr(depth), W, H, C.byref(p), ptr(ws), need, st))
        lib.check(lib.lib.crychic_motion_blur_gather(ctx.handle, ptr(src), ptr(out), W, H, row0, rows, C.byref(p), ptr(ws), need, st))
    s.synchronize()
    planes.verify()
    return ws.cpu().numpy(), out.cpu().numpy().reshape(H, W, 4)
