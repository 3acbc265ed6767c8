"""Builds and loads tests/taa_upscale_ref (TEST INFRASTRUCTURE ONLY): the checker of crychic_taa_upscale, plain C written from the
definition in include/crychic_hip.h with none of the kernel's code; the corpus of matrices, planes, jitters and parameters the host and
the device tests share; and the analytic still scene of the convergence test."""
import ctypes as C
import os

import numpy as np

from post_pass_lib import GUARD, DevicePlanes, build_checker, guarded, guards_intact      # noqa: F401 -- what the post passes' tests share
import taa_lib as ta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "taa_upscale_ref")
SRC, LIB = os.path.join(DIR, "taa_upscale_ref.c"), os.path.join(DIR, "libtaaupscaleref.so")

RESET, NO_CLAMP = ta.RESET, ta.NO_CLAMP
B_HISTORY, B_FX, B_FY, B_CLAMPED = 1, 2, 4, 8           # the bits of the checker's branch plane
DEFAULT_BLEND = 102
WAVE = 8                                                # the kernel's 8 x 8 wavefront tile of output pixels
# (Wi, Hi, Wo, Ho): ratio 1; 1.5 x; unequal, non-integer ratios; 2 x; the limit; every clamp; partial tiles either way; several tiles in a row
SHAPES = ((7, 5, 7, 5), (6, 4, 9, 6), (7, 5, 11, 9), (8, 8, 16, 16), (3, 2, 12, 8), (1, 1, 3, 3), (47, 26, 70, 38), (33, 9, 130, 9))
MOTIONS = ta.MOTIONS


def build():
    return build_checker(SRC, LIB)


def halton(index):
    return ta.jitter(index)


def jitters():
    """Zero, the ends of the range and the first four of the sequence."""
    return [(0.0, 0.0), (0.5, -0.5), (-0.5, 0.5)] + [halton(k) for k in range(4)]


class Case:
    """One call: InvViewProj of the frame's own constants, the two unjittered view-projections (16 floats each, stored transposed), the
    jitter, the (Hi, Wi) uint32 depth plane, the (Hi, Wi, 4) uint8 frame, the (Ho, Wo, 4) uint16 history (None only with RESET), blend
    and flags."""

    def __init__(self, name, ivp, cur, prev, jitter, depth, img, out_size, hist, blend=DEFAULT_BLEND, flags=0):
        self.name = name
        self.ivp, self.cur, self.prev = (np.ascontiguousarray(m, np.float32).reshape(16).copy() for m in (ivp, cur, prev))
        self.jitter = (float(jitter[0]), float(jitter[1]))
        self.depth = np.ascontiguousarray(depth, np.uint32)
        self.img = np.ascontiguousarray(img, np.uint8)
        self.hist = None if hist is None else np.ascontiguousarray(hist, np.uint16)
        self.blend, self.flags = int(blend), int(flags)
        self.Hi, self.Wi = self.img.shape[:2]
        self.Wo, self.Ho = int(out_size[0]), int(out_size[1])
        assert self.depth.shape == (self.Hi, self.Wi) and self.img.shape == (self.Hi, self.Wi, 4)
        assert self.hist is None or self.hist.shape == (self.Ho, self.Wo, 4)
        for a in (self.ivp, self.cur, self.prev, self.depth, self.img) + (() if self.hist is None else (self.hist,)):
            a.setflags(write=False)

    def pass_constants(self, lib):
        """A PassConstants of the product's bindings holding this case's InvViewProj (the rest zero)."""
        pcb = lib.PassConstants()
        pcb.InvViewProj[:] = [float(v) for v in self.ivp]
        return pcb

    def as_taa(self):
        """The crychic_taa case of the same planes (equal sizes only)."""
        assert (self.Wi, self.Hi) == (self.Wo, self.Ho)
        return ta.Case(self.name, self.ivp, self.cur, self.prev, self.depth, self.img, self.hist, self.blend, self.flags)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = C.CDLL(build())
        _REF.taa_upscale_ref.argtypes = ([C.c_void_p] * 3 + [C.c_float] * 2 + [C.c_void_p] * 2 + [C.c_uint32] * 2 + [C.c_void_p] * 3 + [C.c_uint32] * 6 +
                                         [C.c_void_p] * 2)
        _REF.taa_upscale_ref.restype = None
    return _REF


def checker(case, row0=0, rows=None, out=None, hist_out=None, weight=None):
    """(out, history_out, branch): rows [row0, row0 + rows) of the resolved (Ho, Wo, 4) uint8 frame and of the (Ho, Wo, 4) uint16
    history written into `out` and `hist_out` -- planes of 0xA5 bytes by default --, and the (Ho, Wo) uint8 plane of the branch bits of
    the rows' pixels (0 elsewhere).  weight: an (Ho, Wo) uint16 plane that receives each pixel's wgt."""
    Ho, Wo = case.Ho, case.Wo
    rows = Ho - row0 if rows is None else rows
    out = np.full((Ho, Wo, 4), GUARD, np.uint8) if out is None else out
    hist_out = np.full((Ho, Wo, 4), GUARD * 257, np.uint16) if hist_out is None else hist_out
    branch = np.zeros((Ho, Wo), np.uint8)
    _ref().taa_upscale_ref(case.ivp.ctypes.data, case.cur.ctypes.data, case.prev.ctypes.data, case.jitter[0], case.jitter[1], case.depth.ctypes.data,
                           case.img.ctypes.data, case.Wi, case.Hi, None if case.hist is None else case.hist.ctypes.data, hist_out.ctypes.data,
                           out.ctypes.data, Wo, Ho, row0, rows, case.blend, case.flags, branch.ctypes.data,
                           None if weight is None else weight.ctypes.data)
    return out, hist_out, branch


def weights(case):
    """The (Ho, Wo) plane of the weight each output pixel gives the current frame, from the checker."""
    w = np.zeros((case.Ho, case.Wo), np.uint16)
    checker(case, weight=w)
    return w


def vote_case(name, W, H, sx, sy, one_lane, rng):
    """ta.vote_case at ratio 1 under a jitter: the nearest texel of output pixel (ox, oy) is (ox, oy), so exactly one lane of every
    wavefront differs from the rest."""
    c = ta.vote_case(name, W, H, sx, sy, one_lane, rng)
    return Case(name, c.ivp, c.cur, c.prev, (0.25, -0.375), c.depth, c.img, (W, H), c.hist, blend=77)


_CORPUS = {}


def corpus():
    """[Case]: built once and read-only.  Every shape of SHAPES under every jitter and every motion, with depth kinds, history kinds,
    blends and flags rotated through them; the vote planes; RESET frames with and without a history plane."""
    if "cases" in _CORPUS:
        return _CORPUS["cases"]
    rng = np.random.default_rng(28)
    cases = []
    blends = (DEFAULT_BLEND, 1, 256)
    v = 0
    for Wi, Hi, Wo, Ho in SHAPES:
        for ji, jit in enumerate(jitters()):
            for motion in MOTIONS:
                dk = ("random", "ramp", "ones")[v % 3]
                hk = ("random", "near")[(v // 3) % 2]
                blend = blends[(v // 2) % 3]
                flags = (NO_CLAMP if v % 7 == 3 else 0) | (RESET if v % 11 == 5 else 0)
                ivp, cur, prev = ta.motion_matrices(motion, Wi, Hi, jitter=jit)
                img = rng.integers(0, 256, (Hi, Wi, 4), dtype=np.uint8)
                big = np.repeat(np.repeat(img, 4, axis=0), 4, axis=1)[:Ho, :Wo]         # something of the output's shape close to the frame
                cases.append(Case("%dx%d_%dx%d_j%d_%s_%s_%s_b%d_f%d" % (Wi, Hi, Wo, Ho, ji, motion, dk, hk, blend, flags), ivp, cur, prev, jit,
                                  ta.make_depth(dk, Wi, Hi, rng), img, (Wo, Ho), ta.make_history(hk, big, rng), blend, flags))
                v += 1
    # the votes: 64 x 16 is 8 x 2 wavefronts; a shear of half a texel, and one that leaves the frame
    for axis, (sx, sy) in (("fx", (1.0 / 64.0, 0.0)), ("fy", (0.0, 1.0 / 16.0)), ("hist", (8.0, 0.0))):
        for one in (True, False):
            cases.append(vote_case("vote_%s_%s" % (axis, "one_lane" if one else "all_but_one"), 64, 16, sx, sy, one, rng))
    ivp, cur, prev = ta.motion_matrices("dolly", 33, 9)
    img = rng.integers(0, 256, (9, 33, 4), dtype=np.uint8)
    d = ta.make_depth("random", 33, 9, rng)
    cases.append(Case("reset_null_history", ivp, cur, prev, (0.125, 0.25), d, img, (50, 20), None, flags=RESET | NO_CLAMP))
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


wave_counts = ta.wave_counts


# ---- the analytic still scene (the convergence test) ----------------------------------------------------------------------------------

def scene_rgb(u, v):
    """The closed-form image at positions (u, v) in [0, 1]^2 (arrays of one shape): float RGB in 0 .. 255.  A zone plate on the left
    half, slanted stripes whose frequency grows to the right in the upper right quarter, thin bright lines on dark in the lower right."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    zone = 0.5 + 0.5 * np.cos(900.0 * ((u - 0.25) ** 2 + (v * 0.5625 - 0.28) ** 2 * 1.0))
    stripes = (np.floor((u * 1.0 + v * 0.37) * (40.0 + 120.0 * (u - 0.5))) % 2 == 0).astype(np.float64)
    lines = ((np.abs(((u - 0.5) * 3.1 + (v - 0.5) * 1.3) * 37.0 % 1.0 - 0.5) < 0.06) | (np.abs((v * 23.0 + u * 2.0) % 1.0 - 0.5) < 0.05)).astype(np.float64)
    g = np.where(u < 0.5, zone, np.where(v < 0.5, stripes, lines))
    return np.stack([255.0 * g, 255.0 * (0.15 + 0.85 * g) * (0.5 + 0.5 * v), 255.0 * (1.0 - 0.8 * g)], axis=-1)


def analytic_scene(W, H, jitter=(0.0, 0.0)):
    """The (H, W, 4) uint8 frame a W x H render of the scene shows under `jitter`: texel (x, y) of a frame that shows at p + j what
    the unjittered frame shows at p samples the unjittered position (x + 0.5 - jx, y + 0.5 - jy).  Alpha 255."""
    x, y = np.meshgrid(np.arange(W) + 0.5 - jitter[0], np.arange(H) + 0.5 - jitter[1])
    rgb = np.floor(scene_rgb(x / W, y / H) + 0.5)
    return np.concatenate([rgb, np.full((H, W, 1), 255.0)], axis=-1).astype(np.uint8)


def analytic_truth(W, H, ss=8):
    """(H, W, 3) float64: ss x ss supersamples per pixel of the scene, averaged."""
    x, y = np.meshgrid((np.arange(W * ss) + 0.5) / (W * ss), (np.arange(H * ss) + 0.5) / (H * ss))
    return scene_rgb(x, y).reshape(H, ss, W, ss, 3).mean(axis=(1, 3))


def still_sequence(fn, Wi, Hi, Wo, Ho, frames, negate=False, blend=DEFAULT_BLEND, flags=0):
    """The resolved (Ho, Wo, 4) frame after `frames` jittered frames of the analytic scene under a still camera and a constant depth,
    the first a RESET frame; fn(case) -> (out, history_out).  negate: the pass is told the opposite of the jitter the frame was
    rendered with."""
    cur, _ = ta.camera_matrices(Wi, Hi)
    depth = np.full((Hi, Wi), 0xF00000, np.uint32)
    hist, out = None, None
    for k in range(frames):
        jit = halton(k)
        _, ivp = ta.camera_matrices(Wi, Hi, jitter=jit)
        told = (-jit[0], -jit[1]) if negate else jit
        out, hist = fn(Case("still%d" % k, ivp, cur, cur, told, depth, analytic_scene(Wi, Hi, jit), (Wo, Ho), hist, blend,
                            flags | (RESET if hist is None else 0)))[:2]
    return out


def bilinear_frame(Wi, Hi, Wo, Ho):
    """One unjittered frame of the analytic scene upsampled bilinearly: the pass's RESET answer."""
    cur, ivp = ta.camera_matrices(Wi, Hi)
    return checker(Case("bilinear", ivp, cur, cur, (0.0, 0.0), np.full((Hi, Wi), 0xF00000, np.uint32), analytic_scene(Wi, Hi), (Wo, Ho), None,
                        flags=RESET))[0]


def mean_abs_error(frame, truth):
    return float(np.abs(frame[..., :3].astype(np.float64) - truth).mean())


# ---- the device (GPU tier) ------------------------------------------------------------------------------------------------------------

def run_device(dev, case, row0=0, rows=None, misalign=0):
    """crychic_taa_upscale on guarded device copies of the case's planes, the frame planes `misalign` bytes and the history planes
    `misalign & 8` bytes past a 256-byte boundary: (out, history_out) as numpy, the guards and the inputs checked.  dev = (the
    product's _lib module, a Context, torch)."""
    lib, ctx, torch = dev
    Ho, Wo = case.Ho, case.Wo
    planes = DevicePlanes(dev)
    src = planes.upload("input", case.img, misalign)
    depth = planes.upload("depth", case.depth, misalign)
    out = planes.blank("out", (Ho, Wo, 4), np.uint8, misalign)
    hout = planes.blank("history out", (Ho, Wo, 4), np.uint16, misalign & 8)
    hin = None if case.hist is None else planes.upload("history in", case.hist, misalign & 8)
    pcb = case.pass_constants(lib)
    p = lib.TaaUpscaleParams.default(blend=case.blend, flags=case.flags)
    cur, prev = (C.c_float * 16)(*case.cur), (C.c_float * 16)(*case.prev)
    s = torch.cuda.current_stream(ctx.device)
    lib.check(lib.lib.crychic_taa_upscale(ctx.handle, C.byref(pcb), cur, prev, case.jitter[0], case.jitter[1], C.c_void_p(depth.data_ptr()),
                                          C.c_void_p(src.data_ptr()), case.Wi, case.Hi, None if hin is None else C.c_void_p(hin.data_ptr()),
                                          C.c_void_p(hout.data_ptr()), C.c_void_p(out.data_ptr()), Wo, Ho, row0, Ho - row0 if rows is None else rows,
                                          C.byref(p), C.c_void_p(s.cuda_stream)))
    s.synchronize()
    planes.verify()
    return out.cpu().numpy().reshape(Ho, Wo, 4), hout.cpu().numpy().view(np.uint16).reshape(Ho, Wo, 4)


# ---- the definition's integer front end restated in numpy, and the known answers the host and the device tests share ------------------

def np_current(case):
    """(c256 (Ho, Wo, 3) int64, cA (Ho, Wo) int64, wgt (Ho, Wo) int64): steps 1 to 3 of the definition in numpy's 64-bit integers."""
    def axis(No, Ni, j):
        J = int(np.floor(np.float64(np.float32(j)) * 256.0 + 0.5))
        U = ((2 * np.arange(No, dtype=np.int64) + 1) * Ni * 256) // (2 * No) + J - 128
        i, f = U >> 8, U & 255
        d = np.minimum(256, (np.minimum(f, 256 - f) * No) // Ni)
        return np.clip(i, 0, Ni - 1), np.clip(i + 1, 0, Ni - 1), f, np.clip((U + 128) >> 8, 0, Ni - 1), 256 - d
    x0, x1, fu, tx, nx = axis(case.Wo, case.Wi, case.jitter[0])
    y0, y1, fv, ty, ny = axis(case.Ho, case.Hi, case.jitter[1])
    img = case.img.astype(np.int64)
    fu, fv = fu[None, :, None], fv[:, None, None]
    top = img[y0][:, x0, :3] * (256 - fu) + img[y0][:, x1, :3] * fu
    bot = img[y1][:, x0, :3] * (256 - fu) + img[y1][:, x1, :3] * fu
    c256 = (top * (256 - fv) + bot * fv + 128) >> 8
    conf = (ny[:, None] * nx[None, :]) >> 8
    wgt = np.minimum(256, (case.blend * ((conf * conf) >> 8)) >> 8)
    return c256, img[ty][:, tx, 3], wgt


def answers(fn):
    """The definition's known answers for fn(case) -> (out, history_out)."""
    rng = np.random.default_rng(6)
    # RESET: history_out == c256 and out == the rounded bilinear frame, whatever the history, the sizes and the jitter
    for (Wi, Hi, Wo, Ho), jit in zip(SHAPES, jitters() + [(0.0, 0.0)]):
        img = rng.integers(0, 256, (Hi, Wi, 4), dtype=np.uint8)
        ivp, cur, prev = ta.motion_matrices("dolly", Wi, Hi, jitter=jit)
        for hist in (rng.integers(0, 1 << 16, (Ho, Wo, 4), dtype=np.uint16), None):
            case = Case("reset", ivp, cur, prev, jit, ta.make_depth("random", Wi, Hi, rng), img, (Wo, Ho), hist, flags=RESET)
            out, hout = fn(case)
            c256, cA, _ = np_current(case)
            assert np.array_equal(hout[..., :3], c256) and np.array_equal(hout[..., 3], 256 * cA), (Wi, Hi, Wo, Ho)
            assert np.array_equal(out[..., :3], np.minimum((c256 + 128) >> 8, 255)) and np.array_equal(out[..., 3], cA), (Wi, Hi, Wo, Ho)
    # equal sizes, zero jitter: crychic_taa with the same blend, byte for byte
    for W, H in ((7, 5), (70, 38)):
        for motion in MOTIONS:
            for blend, flags in ((DEFAULT_BLEND, 0), (26, NO_CLAMP), (256, 0)):
                img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
                ivp, cur, prev = ta.motion_matrices(motion, W, H, jitter=(0.0, 0.0))
                case = Case("ratio1", ivp, cur, prev, (0.0, 0.0), ta.make_depth("random", W, H, rng), img, (W, H), ta.make_history("near", img, rng), blend, flags)
                out, hout = fn(case)
                want_out, want_hist, _ = ta.checker(case.as_taa())
                assert np.array_equal(out, want_out) and np.array_equal(hout, want_hist), (W, H, motion, blend, flags)
    # a constant frame over a constant history with identical matrices and NO_CLAMP: the closed form with each pixel's own weight
    Cc, Hc = np.array([200, 17, 96, 33], np.int64), np.array([1234, 65535, 24576, 999], np.int64)
    for (Wi, Hi, Wo, Ho), jit in zip(SHAPES, jitters() + [(0.0, 0.0)]):
        flat = np.broadcast_to(Cc.astype(np.uint8), (Hi, Wi, 4)).copy()
        flat_h = np.broadcast_to(Hc.astype(np.uint16), (Ho, Wo, 4)).copy()
        ivp, cur, _ = ta.motion_matrices("identical", Wi, Hi, jitter=jit)
        for blend in (1, DEFAULT_BLEND, 256):
            case = Case("flat", ivp, cur, cur, jit, ta.make_depth("ramp", Wi, Hi, rng), flat, (Wo, Ho), flat_h, blend, NO_CLAMP)
            out, hout = fn(case)
            wgt = np_current(case)[2][..., None]
            nn = (Hc[:3] * (256 - wgt) + Cc[:3] * 256 * wgt + 128) >> 8
            assert np.array_equal(hout[..., :3], nn) and (hout[..., 3] == 256 * 33).all(), (Wi, Hi, Wo, Ho, blend)
            assert np.array_equal(out[..., :3], np.minimum((nn + 128) >> 8, 255)) and (out[..., 3] == 33).all(), (Wi, Hi, Wo, Ho, blend)
            # with the clamp the history is pulled to the frame: out == C
            out, hout = fn(Case("flat_clamp", ivp, cur, cur, jit, case.depth, flat, (Wo, Ho), flat_h, blend, 0))
            assert (out == Cc).all() and (hout == Cc * 256).all()
    # 2 x with zero jitter: conf2 == 16 in every pixel, so wgt == (blend 16) >> 8
    Wi, Hi, Wo, Ho = 8, 8, 16, 16
    flat = np.broadcast_to(Cc.astype(np.uint8), (Hi, Wi, 4)).copy()
    flat_h = np.broadcast_to(Hc.astype(np.uint16), (Ho, Wo, 4)).copy()
    ivp, cur, _ = ta.motion_matrices("identical", Wi, Hi, jitter=(0.0, 0.0))
    for blend in (DEFAULT_BLEND, 256):
        wgt = (blend * 16) >> 8
        out, hout = fn(Case("two_times", ivp, cur, cur, (0.0, 0.0), ta.make_depth("ones", Wi, Hi, rng), flat, (Wo, Ho), flat_h, blend, NO_CLAMP))
        assert (hout[..., :3] == (Hc[:3] * (256 - wgt) + Cc[:3] * 256 * wgt + 128) >> 8).all(), blend
