"""Builds and loads tests/dof_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_dof, plain C written from the definition in
include/crychic_hip.h with none of the kernel's code; and the corpus of frames, images and parameter sets the host and the device
tests share."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "dof_ref")
SRC, LIB = os.path.join(DIR, "dof_ref.c"), os.path.join(DIR, "libdofref.so")
GOLD = os.path.join(ROOT, "tests", "golden", "frame_64x64.npz")

COUNTERS = ("tap_outside", "behind", "not_behind", "k_zero", "k_interior", "k_sixteen", "ce_below_16", "ce_in_inv", "c_zero", "c_interior", "c_hi",
            "clamp_nan")
DEFAULTS = dict(focus=15.0, aperture=6.0, radius=8)
# every R of {1, 2, 5, 8} and every aperture of {0, 0.5, 6, 64} with a focus distance in front of the reference scene (its boxes stand
# 5 .. 40 units from the eye), inside it and behind it; nan_clamp: g = focus / B overflows to -inf, x = +inf, e = +inf and
# u = inf * 0 is NaN (only with the B of nan_frame)
PARAM_SETS = {
    "default": DEFAULTS,
    "copy_r8": dict(focus=15.0, aperture=0.0, radius=8),
    "front_thin_r1": dict(focus=2.0, aperture=0.5, radius=1),
    "behind_wide_r5": dict(focus=90.0, aperture=64.0, radius=5),
    "inside_wide_r2": dict(focus=15.0, aperture=64.0, radius=2),
    "front_r5": dict(focus=2.0, aperture=6.0, radius=5),
    "behind_thin_r8": dict(focus=90.0, aperture=0.5, radius=8),
    "inside_wide_r8": dict(focus=10.0, aperture=64.0, radius=8),
    "behind_r1": dict(focus=100.0, aperture=6.0, radius=1),
    "inside_r2": dict(focus=8.0, aperture=6.0, radius=2),
    "copy_r2": dict(focus=40.0, aperture=0.0, radius=2),
    "far_focus_wide_r8": dict(focus=100.0, aperture=64.0, radius=8),
    "nan_clamp": dict(focus=3.0e38, aperture=0.0, radius=8),
}
# widths and heights either side of the 64 x 16 tile and of the 32 x 32 one, with and without room for the apron, degenerate frames,
# and one frame of several workgroups each way
SIZES = ((1, 1), (3, 5), (63, 4), (64, 4), (65, 7), (130, 9), (322, 190))
DEPTH_KINDS = ("zeros", "ones", "random", "step_near_left", "step_near_right")


def build():
    return build_checker(SRC, LIB)


def f32(x):
    return float(np.float32(x))


def projection(near, far):
    """(A, B) = (Proj[10], Proj[11]) of a perspective projection, in binary32: viewZ = B / (d - A)."""
    n, f = np.float32(near), np.float32(far)
    return f32(f / (f - n)), f32(-n * f / (f - n))


REFERENCE_AB = projection(1.0, 100.0)           # the reference camera's near and far planes (d3dApp / Camera::SetLens)
OTHER_AB = projection(0.5, 500.0)


def depth_word(ab, view_z):
    """The D24 word of view-space distance view_z under (A, B)."""
    d = ab[0] + ab[1] / view_z
    return int(min(max(round(d * 16777215.0), 0), 0xFFFFFF))


class Frame:
    """What the pass reads besides the image: A = Proj[10], B = Proj[11] and the (H, W) uint32 depth plane."""

    def __init__(self, ab, depth):
        self.A, self.B = f32(ab[0]), f32(ab[1])
        self.depth = np.ascontiguousarray(depth, np.uint32)

    @classmethod
    def from_pass_cb(cls, pcb, depth):
        """pcb: a PassConstants (any ctypes object or buffer of its bytes); Proj starts at float 32."""
        f = np.frombuffer(bytes(pcb), np.float32)
        return cls((f[42], f[43]), depth)

    def pass_constants(self, lib):
        """A PassConstants of the product's bindings holding this frame's two numbers (the rest zero)."""
        pcb = lib.PassConstants()
        pcb.Proj[10], pcb.Proj[11] = self.A, self.B
        return pcb

    def proj(self):
        p = np.zeros(16, np.float32)
        p[10], p[11] = self.A, self.B
        return p


def consts_array(frame, params=None):
    """{ A, B, focusDistance, aperture } as float bits: what dof_ref takes."""
    p = dict(DEFAULTS, **(params or {}))
    return np.array([frame.A, frame.B, p["focus"], p["aperture"]], np.float32).view(np.uint32), int(p["radius"])


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.dof_ref.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
        _REF.dof_ref.restype = None
        _REF.dof_ref_coc.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        for fn in (_REF.dof_ref_coc, _REF.dof_ref_disc, _REF.dof_ref_inv, _REF.dof_ref_d16):
            fn.restype = C.c_uint32
        _REF.dof_ref_disc.argtypes = _REF.dof_ref_inv.argtypes = [C.c_uint32]
        _REF.dof_ref_d16.argtypes = [C.c_int, C.c_int]
    return _REF


def checker(frame, img, params=None, row0=0, rows=None, out=None, coc=False):
    """(rows [row0, row0 + rows) of the blurred (H, W, 4) uint8 frame `img` written into `out` -- a frame of 0xA5 by default --,
    {counter: count over those rows}); with coc=True a third value, the (H, W) uint32 plane of c (0 outside the rows)."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    assert frame.depth.shape == (H, W)
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), GUARD, np.uint8) if out is None else out
    n = np.zeros(len(COUNTERS), np.uint64)
    cc = np.zeros((H, W), np.uint32) if coc else None
    k, R = consts_array(frame, params)
    _ref().dof_ref(k.ctypes.data, R, frame.depth.ctypes.data, img.ctypes.data, out.ctypes.data, W, H, row0, rows, n.ctypes.data,
                   None if cc is None else cc.ctypes.data)
    counts = dict(zip(COUNTERS, (int(v) for v in n)))
    return (out, counts, cc) if coc else (out, counts)


def coc_of(frame, params, word):
    k, R = consts_array(frame, params)
    return int(_ref().dof_ref_coc(k.ctypes.data, R, int(word), None))


def tables():
    """(disc sizes at R = 1 .. 8, inv[0 .. 128], {(ox, oy): d16} of the radius-8 disc) from the checker's own functions."""
    r = _ref()
    d16 = {(ox, oy): int(r.dof_ref_d16(ox, oy)) for oy in range(-8, 9) for ox in range(-8, 9) if ox * ox + oy * oy <= 64}
    return [int(r.dof_ref_disc(R)) for R in range(1, 9)], [int(r.dof_ref_inv(c)) for c in range(129)], d16


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

def make_depth(kind, W, H, rng, ab=REFERENCE_AB):
    if kind == "zeros":
        return np.zeros((H, W), np.uint32)
    if kind == "ones":
        return np.full((H, W), 0xFFFFFF, np.uint32)
    if kind == "random":
        return rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)                # 24 random bits and a random top byte
    # the depth step of the known answers: 10 units from the eye on one side of the middle column, the far plane on the other
    near, far = depth_word(ab, 10.0) | 0x5A000000, 0xFFFFFF
    d = np.full((H, W), far, np.uint32)
    if kind == "step_near_left":
        d[:, :W // 2] = near
    else:
        d[:, W // 2:] = near
    return d


def golden_frame():
    """The committed 64 x 64 frame: its depth plane and pass constants, and the frame lit from them."""
    g = np.load(GOLD, allow_pickle=False)
    return Frame.from_pass_cb(g["pass_cb"].tobytes(), g["depth"]), np.ascontiguousarray(g["lit_3light_intended_sky"])


_SCENE = {}


def scene_frame():
    """The 128 x 96 synthetic scene (crychic_renderer_amd.scene, on the CPU): its depth plane and pass constants."""
    if "frame" not in _SCENE:
        from crychic_renderer_amd import scene
        planes = scene.make_scene(128, 96, shadow_dim=64, cube_dim=8, device="cpu")
        _SCENE["frame"] = Frame.from_pass_cb(planes["consts"].pass_cb, planes["depth"].numpy().view(np.uint32))
    return _SCENE["frame"]


_CORPUS = {}


def corpus():
    """[(name, Frame, image, parameter-set name, depth kind)]: built once and read-only.  The rendered frames under every parameter
    set; every size of SIZES under every depth kind, the parameter sets and the two projections taken in turn."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    rng = np.random.default_rng(21)
    cases = []
    gold, lit = golden_frame()
    sc = scene_frame()
    sc_img = rng.integers(0, 256, (96, 128, 4), dtype=np.uint8)
    names = [n for n in PARAM_SETS if n != "nan_clamp"]
    for pname in names:
        cases.append(("golden64_" + pname, gold, lit, pname, "rendered"))
        cases.append(("scene128_" + pname, sc, sc_img, pname, "rendered"))
    turn = 0
    for W, H in SIZES:
        for dk in DEPTH_KINDS:
            ab = (REFERENCE_AB, OTHER_AB)[turn % 2]
            pname = names[(5 * turn + 3) % len(names)]
            turn += 1
            img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            cases.append(("%dx%d_%s_%s_%s" % (W, H, dk, "ref" if ab is REFERENCE_AB else "other", pname), Frame(ab, make_depth(dk, W, H, rng, ab)), img, pname, dk))
    # the two steps under the parameters of the known answers, on the frame of several workgroups
    img = rng.integers(0, 256, (190, 322, 4), dtype=np.uint8)
    cases.append(("322x190_step_near_sharp", Frame(REFERENCE_AB, make_depth("step_near_left", 322, 190, rng)), img, "inside_wide_r8", "step_near_left"))
    cases.append(("322x190_step_near_blurred", Frame(REFERENCE_AB, make_depth("step_near_right", 322, 190, rng)), img, "far_focus_wide_r8", "step_near_right"))
    # the NaN path of the clamp: B so small that g overflows
    img = rng.integers(0, 256, (7, 65, 4), dtype=np.uint8)
    cases.append(("nan_clamp", Frame((REFERENCE_AB[0], -1.0e-3), make_depth("random", 65, 7, rng)), img, "nan_clamp", "random"))
    for _, frame, im, _, _ in cases:
        frame.depth.setflags(write=False)
        im.setflags(write=False)
    _CORPUS["cases"] = cases
    return cases


def case_name(prefix):
    """The one corpus case whose name starts with `prefix`."""
    found = [c[0] for c in corpus() if c[0].startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    return found[0]


_EXPECTED = {}


def expected(name):
    """The checker's whole frame and counters for corpus case `name`; computed once, read-only."""
    if name not in _EXPECTED:
        case = {c[0]: c for c in corpus()}[name]
        out, n = checker(case[1], case[2], PARAM_SETS[case[3]])
        out.setflags(write=False)
        _EXPECTED[name] = (out, n)
    return _EXPECTED[name]
