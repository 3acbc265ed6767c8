"""The constant sets that drive every host guard of the SSAO pass and the blur chain across its threshold
(tests/test_ssao_guards_host.py, tests/test_ssao_guards_gpu.py).

The guards (ssao_core.hpp ssao_projtex_is_sparse / ssao_sky_reach / ssao_cull_params, blur_tiles.hpp blur_weights_positive) switch
shortcuts that are exact only under conditions on crychic_ssao_constants.  A case is one constant set with a frame generated from
ITS OWN projection, what each guard must decide for it (`expect`, written down here from the conditions, never read back from the
code) and which shortcut counters of the host build must be non-zero on its frame (`bites`).  Values sit on both sides of every
inequality, as close as binary32 allows: where a guard compares in double, the two float neighbours of the threshold are taken
(the little arithmetic that finds them -- farZ = B / (1 - A), D = |R| max|offset| 7 * 1.001 -- only chooses inputs).

Frames (fuzz_util's probes, at sizes the device tests may use too):
  clear  640 x 384  sky with patches next to the far plane, geometry hugging the near plane, taps at and behind the camera,
                    non-finite normals: the sky exit, tap culling and the clear-cell rule all fire on it
  sky    640 x 384  the sky field with patches in cell corners alone (the reach bound's worst case)
  cull   384 x 224  the reference scene through the case's camera, with spikes and holes
  wall   322 x 190  a rough wall, ragged tile grid: every texel changes under the blur
  wallsky 640 x 384 the wall with blocks of sky: blur tiles settle there"""
import copy
import ctypes as C
import math

import numpy as np

f32 = np.float32
GUARDS = ("sparse", "sky", "cull", "clear", "weights")
COUNTERS = ("sky_waves", "culled_taps", "clear_cell_taps", "settled_tiles")
FRAME_SIZE = {"clear": (640, 384), "sky": (640, 384), "cull": (384, 224), "wall": (322, 190), "wallsky": (640, 384)}
# seeds of fuzz_util's builders: clear 3 and sky 15 scatter infinite normals (their pixels come out NaN -> 0 whatever the constants
# are, and keep their wavefronts off the sky exit), sky 15 hugs cell corners with the longest reflected offsets; wallsky 3 settles
# 19 blur tiles at three iterations
FRAME_SEED = {"clear": 3, "sky": 15, "cull": 1, "wall": 1, "wallsky": 3}
REF_CAM = (1.0, 100.0, 0.25 * math.pi)          # near, far, fovY of the reference camera
BLUR_COUNT = 3


def up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def down(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


def far_z(cb):
    return float(cb.Proj[11]) / (1.0 - float(cb.Proj[10]))


def max_offset(cb):
    return max(math.sqrt(sum(float(cb.OffsetVectors[i][k]) ** 2 for k in range(3))) for i in range(14))


# ---- edits of a constant buffer (each returns a function of cb) ------------------------------------------------------------------
def field(name, value):
    def f(cb):
        setattr(cb, name, value)
    return f


def elem(name, index, value):
    def f(cb):
        getattr(cb, name)[index] = value
    return f


def eps_at_threshold(side):
    """SurfaceEpsilon = the largest float not above farZ * 2^-16 (side 0: the guards' `eps > farZ * 2^-16` fails) or the next one."""
    def f(cb):
        thr = far_z(cb) * 2.0 ** -16
        lo = f32(thr)
        if float(lo) > thr:
            lo = np.nextafter(lo, f32(0.0))
        assert float(lo) <= thr < up(lo)
        cb.SurfaceEpsilon = float(lo) if side == 0 else up(lo)
    return f


def radius_at_reach(side):
    """OcclusionRadius = the largest float with D < 0.5 farZ (side 0) or the next one (side 1: the sky exit's reach is unbounded)."""
    def f(cb):
        half, omax = 0.5 * far_z(cb), max_offset(cb)
        D = lambda r: float(r) * omax * 7.0 * 1.001
        r = f32(half / (omax * 7.0 * 1.001))
        while not D(r) < half:
            r = np.nextafter(r, f32(0.0))
        while D(np.nextafter(r, f32(np.inf))) < half:
            r = np.nextafter(r, f32(np.inf))
        cb.OcclusionRadius = float(r) if side == 0 else up(r)
    return f


def far_at_1e6(side):
    """Proj's B = the float that puts farZ = B / (1 - A) just under 1e6 (side 0) or the next one down (farZ >= 1e6)."""
    def f(cb):
        A = float(cb.Proj[10])
        b = f32((1.0 - A) * 1.0e6)                      # negative
        fz = lambda v: float(v) / (1.0 - A)
        while not fz(b) < 1.0e6:
            b = np.nextafter(b, f32(0.0))
        while fz(np.nextafter(b, f32(-np.inf))) < 1.0e6:
            b = np.nextafter(b, f32(-np.inf))
        cb.Proj[11] = float(b) if side == 0 else down(b)
    return f


def scale_offsets(s):
    def f(cb):
        for i in range(14):
            for k in range(4):
                cb.OffsetVectors[i][k] = float(cb.OffsetVectors[i][k]) * s
    return f


def offset(i, k, value):
    def f(cb):
        cb.OffsetVectors[i][k] = value
    return f


def weights(values):
    values = [float(v) for v in values]
    assert len(values) == 11

    def f(cb):
        flat = C.cast(cb.BlurWeights, C.POINTER(C.c_float))
        for i, v in enumerate(values):
            flat[i] = v
    return f


def one_weight(i, value):
    def f(cb):
        C.cast(cb.BlurWeights, C.POINTER(C.c_float))[i] = value
    return f


def gauss_padded(sigma):
    """crychic_calc_gauss_weights(sigma) centred in the 11 slots, zeros around it (a narrower Gaussian of an integrator)."""
    def f(cb):
        from crychic_renderer_amd._lib import lib
        w = (C.c_float * 11)()
        n = 2 * int(math.ceil(2.0 * sigma)) + 1
        assert lib.crychic_calc_gauss_weights(sigma, w, 11) == n
        pad = (11 - n) // 2
        weights([0.0] * pad + [w[i] for i in range(n)] + [0.0] * (11 - n - pad))(cb)
    return f


def scaled_world(B):
    """The same frame in other units: Proj's B set to `B` and every length of the constants scaled by B / (the old B)."""
    def f(cb):
        s = B / float(cb.Proj[11])
        cb.Proj[11] = B
        for name in ("OcclusionRadius", "OcclusionFadeStart", "OcclusionFadeEnd", "SurfaceEpsilon"):
            setattr(cb, name, float(getattr(cb, name)) * s)
    return f


def several(*edits):
    def f(cb):
        for e in edits:
            e(cb)
    return f


# ---- the table -------------------------------------------------------------------------------------------------------------------
class GuardCase:
    """name; frame: a key of FRAME_SIZE; cam: (near, far, fovY); pre: an edit of the constants the frame is generated FROM (a
    projection a camera cannot express exactly); post: an edit applied after the frame exists; expect: guard -> 0 / 1;
    bites: counters that must be non-zero on the host build (the others of a guard that is on are not asserted; every counter of a
    guard that is off must be exactly zero); blur: the case is about the blur (its blurred map must differ from its raw one)."""

    def __init__(self, name, frame, expect, cam=REF_CAM, pre=None, post=None, bites=None, sky_bites=False, blur=False, seed=None):
        self.name, self.frame, self.cam, self.pre, self.post, self.blur = name, frame, cam, pre, post, blur
        self.seed = FRAME_SEED[frame] if seed is None else seed
        self.expect = dict({g: 1 for g in GUARDS}, **expect)
        assert set(self.expect) == set(GUARDS)
        if bites is None:
            bites = {"clear": ("culled_taps", "clear_cell_taps"), "sky": ("sky_waves", "culled_taps"), "cull": ("culled_taps",),
                     "wall": ("culled_taps",), "wallsky": ("sky_waves", "culled_taps", "settled_tiles")}[frame]
        if sky_bites:                # on the clear frame the sky exit fires only where the reach is short
            bites = ("sky_waves",) + tuple(bites)
        on = {"sky_waves": self.expect["sky"], "culled_taps": self.expect["cull"], "clear_cell_taps": self.expect["clear"],
              "settled_tiles": self.expect["weights"]}
        self.bites = tuple(b for b in bites if on[b])
        self.must_be_zero = tuple(b for b in COUNTERS if not on[b])

    def __repr__(self):
        return self.name


T_A = float(f32(1.000002))                 # ssao_cull_params: A > 1.000002f
BIG = float(f32(1.0e12))                   # ssao_projtex_is_sparse: abs(x) < 1.0e12f
W_MAX = float(f32(1.0e30))                 # blur_weights_positive: w < 1.0e30f; ssao_cull_params: abs(eps) < 1.0e30f
NO_CULL = dict(cull=0, clear=0)
NO_SKY_CLEAR = dict(sky=0, clear=0)
ALL_OFF = dict(sky=0, cull=0, clear=0)
GENERAL = dict(sparse=0, sky=0)
PI4 = REF_CAM[2]


def _cases():
    c = []
    add = lambda *a, **k: c.append(GuardCase(*a, **k))
    # -- projection: cameras ---------------------------------------------------------------------------------------------------
    add("proj_reference", "clear", {})
    # A = far / (far - near) in binary32: 1 + 21 ulp, 1 + 17 ulp (= 1.000002f itself: not above it), 1 + 14 ulp, 1 + 8 ulp.
    # farZ * 2^-16 is 3.05, 3.8, 4.6, 0.153 against SurfaceEpsilon 0.05: no sky exit, no clear cells
    add("proj_A_21ulp", "clear", NO_SKY_CLEAR, cam=(0.5, 200000.0, PI4))
    add("proj_A_17ulp", "clear", ALL_OFF, cam=(0.5, 250000.0, PI4))
    add("proj_A_14ulp", "clear", ALL_OFF, cam=(0.5, 300000.0, PI4))
    add("proj_A_8ulp", "clear", ALL_OFF, cam=(0.01, 1.0e4, PI4))
    add("proj_A_8ulp_eps_half", "clear", NO_CULL, cam=(0.01, 1.0e4, PI4), post=field("SurfaceEpsilon", 0.5), sky_bites=True)      # sky exit without culling
    add("proj_A_8ulp_cull", "cull", ALL_OFF, cam=(0.01, 1.0e4, PI4))
    add("proj_A_21ulp_cull", "cull", NO_SKY_CLEAR, cam=(0.5, 200000.0, PI4))
    # A written: exactly 1.000002f and the float above it (near 0.001, far about 490: farZ * 2^-16 = 0.0075 < 0.05)
    add("proj_A_at_threshold", "clear", NO_CULL, cam=(0.001, 500.0, PI4), pre=elem("Proj", 10, T_A), sky_bites=True)
    add("proj_A_above_threshold", "clear", {}, cam=(0.001, 500.0, PI4), pre=elem("Proj", 10, up(T_A)), sky_bites=True)
    add("proj_A_1ulp", "clear", ALL_OFF, cam=(0.001, 500.0, PI4), pre=elem("Proj", 10, up(1.0)))      # farZ = 8400: 0.128 > SurfaceEpsilon
    # farZ on both sides of 1e6 (near 100; SurfaceEpsilon 16 > 1e6 * 2^-16 = 15.26)
    add("proj_far_under_1e6", "clear", {}, cam=(100.0, 1.0e6, PI4), pre=far_at_1e6(0), post=field("SurfaceEpsilon", 16.0), sky_bites=True)
    add("proj_far_over_1e6", "clear", NO_SKY_CLEAR, cam=(100.0, 1.0e6, PI4), pre=far_at_1e6(1), post=field("SurfaceEpsilon", 16.0))
    # A about 8.4; a radius of 0.5 is D = 3.2 of the 3.35 allowed: the sky exit is on with a reach wider than the frame
    add("proj_short_frustum", "wallsky", {}, cam=(5.9, 6.7, PI4), bites=("culled_taps", "settled_tiles"))
    # fields of view.  At 0.02 (PT[0] = 30, corner slope 0.0167, max|offset| 0.92196) dx = 640 * 30 * 1.0167 * D / (100 - D) with
    # D = 6.4602 R: 4087 texels at a radius of 2.68, 4105 > 4096 at 2.69 (dy is 0.7 % shorter)
    add("proj_fov_0.02_dx_over", "clear", dict(sky=0), cam=(1.0, 100.0, 0.02), post=field("OcclusionRadius", 2.69))
    add("proj_fov_0.02_dx_under", "clear", {}, cam=(1.0, 100.0, 0.02), post=field("OcclusionRadius", 2.68))
    add("proj_fov_0.02", "clear", dict(sky=0), cam=(1.0, 100.0, 0.02))                             # the frame's own radius of 3
    add("proj_fov_3.0", "clear", {}, cam=(1.0, 100.0, 3.0), sky_bites=True)
    add("proj_fov_3.12", "clear", {}, cam=(1.0, 100.0, 3.12), sky_bites=True)
    # -- projection: written into the buffer (the frame is the reference camera's) -----------------------------------------------
    add("proj_B_positive", "clear", ALL_OFF, post=elem("Proj", 11, 1.0101))
    # B at -1e12: the reference scene in units of 1e-12 (radius, fades and epsilon scaled like B, so that it occludes as ever); farZ = 1e14
    add("proj_B_at_-1e12", "cull", ALL_OFF, post=scaled_world(-BIG))
    add("proj_B_above_-1e12", "cull", NO_SKY_CLEAR, post=scaled_world(up(-BIG)))
    add("proj_B_-1.5e12", "cull", ALL_OFF, post=scaled_world(-1.5e12))
    add("proj_A_one", "clear", ALL_OFF, post=elem("Proj", 10, 1.0))                               # farZ = -inf
    add("proj_A_half", "clear", ALL_OFF, post=elem("Proj", 10, 0.5))
    add("proj_A_1e6", "clear", ALL_OFF, post=elem("Proj", 10, 1.0e6))
    add("proj_A_under_1e6", "clear", dict(sky=0), post=elem("Proj", 10, down(1.0e6)))             # farZ = 1e-6: D is not below half of it
    add("proj_invproj_corner_zero", "clear", dict(sky=0), post=elem("InvProj", 8, 1.0))           # ph[2] = 1 - 1 at the left corners
    # (a corner just over 1e-12 has a view-ray slope of 1e12 and fails dx < 4096 instead: the nearest corner that passes is a coarse one)
    add("proj_invproj_corner_half", "clear", {}, post=elem("InvProj", 8, 0.5))                    # ph[2] = 0.5: slopes doubled
    # -- SurfaceEpsilon --------------------------------------------------------------------------------------------------------
    for far in (100.0, 1000.0):
        add("eps_under_far_%g" % far, "clear", NO_SKY_CLEAR, cam=(1.0, far, PI4), post=eps_at_threshold(0))
        add("eps_over_far_%g" % far, "clear", {}, cam=(1.0, far, PI4), post=eps_at_threshold(1), sky_bites=far == 1000.0)
    # (without clear cells nothing on the sky frame is culled: its patches are rough and stand alone)
    add("eps_under_sky", "sky", NO_SKY_CLEAR, post=eps_at_threshold(0), bites=())
    add("eps_over_sky", "sky", {}, post=eps_at_threshold(1))
    # on the sky frame a sky pixel's distZ (rounding noise of the far distance) is above an epsilon of 0: it IS occluded there
    add("eps_zero_sky", "sky", NO_SKY_CLEAR, post=field("SurfaceEpsilon", 0.0), bites=())
    add("eps_negative_sky", "sky", NO_SKY_CLEAR, post=field("SurfaceEpsilon", -0.05), bites=())
    add("eps_zero", "clear", NO_SKY_CLEAR, post=field("SurfaceEpsilon", 0.0))
    add("eps_negative", "clear", NO_SKY_CLEAR, post=field("SurfaceEpsilon", -0.05))
    add("eps_9e29", "clear", {}, post=field("SurfaceEpsilon", 9.0e29))
    add("eps_1e30", "clear", NO_CULL, post=field("SurfaceEpsilon", W_MAX))
    add("eps_under_1e30", "clear", {}, post=field("SurfaceEpsilon", down(W_MAX)))
    add("eps_inf", "clear", NO_CULL, post=field("SurfaceEpsilon", math.inf))
    add("eps_nan", "clear", ALL_OFF, post=field("SurfaceEpsilon", math.nan))
    add("eps_zero_cull", "cull", NO_SKY_CLEAR, post=field("SurfaceEpsilon", 0.0), seed=2)
    # -- reach -----------------------------------------------------------------------------------------------------------------
    add("reach_D_under", "clear", {}, post=radius_at_reach(0))
    add("reach_D_over", "clear", dict(sky=0), post=radius_at_reach(1))
    # D just under half the far distance reaches across the whole frame (rx = 791 of 640 texels): the exit is on and no wavefront
    # can take it; a radius of 1.5 is the nearest that still does
    add("reach_D_under_sky", "sky", {}, post=radius_at_reach(0), bites=("culled_taps",))
    add("reach_radius_1.5_sky", "sky", {}, post=field("OcclusionRadius", 1.5))
    add("reach_D_over_sky", "sky", dict(sky=0), post=radius_at_reach(1))
    # a scaled sample kernel: max|offset| is 0.92196, so D = 0.5 * 15.4 * 0.92196 * 7.007 = 49.74 < 50 < 50.39 (15.6)
    add("reach_offsets_x15.4", "clear", {}, post=several(field("OcclusionRadius", 0.5), scale_offsets(15.4)))
    add("reach_offsets_x15.6", "clear", dict(sky=0), post=several(field("OcclusionRadius", 0.5), scale_offsets(15.6)))
    add("reach_negative_radius", "clear", {}, post=field("OcclusionRadius", -0.5), sky_bites=True)
    add("reach_negative_radius_sky", "sky", {}, post=field("OcclusionRadius", -0.5))
    add("reach_radius_under_1e12", "clear", dict(sky=0), post=field("OcclusionRadius", down(BIG)))
    add("reach_radius_1e12", "clear", GENERAL, post=field("OcclusionRadius", BIG))
    add("reach_radius_-1e12", "clear", GENERAL, post=field("OcclusionRadius", -BIG))
    add("reach_offset_under_1e12", "clear", dict(sky=0), post=offset(3, 1, down(BIG)))
    add("reach_offset_1e12", "clear", GENERAL, post=offset(3, 1, BIG))
    add("reach_offset_-1e12", "clear", GENERAL, post=offset(13, 2, -BIG))
    add("reach_offset_nan", "clear", GENERAL, post=offset(5, 0, math.nan))
    add("reach_offset_nan_cull", "cull", GENERAL, post=offset(0, 2, math.nan))
    # (a NaN tap adds +0 under either gProjTex product and max|offset| skips it: only the sky frame's counter can tell that it passed)
    add("reach_offset_nan_sky", "sky", GENERAL, post=offset(13, 1, math.nan))
    # all offsets zero: every tap is the pixel itself and distZ is rounding noise -- nothing occludes unless SurfaceEpsilon is negative,
    # which switches the sky exit off; offsets of 1e-3 are the nearest that keep it on (D = 0.02) with pixels that come out NaN
    add("reach_offsets_zero", "clear", NO_SKY_CLEAR, post=several(scale_offsets(0.0), field("SurfaceEpsilon", -0.05)), bites=())
    add("reach_offsets_x0.001", "clear", {}, post=scale_offsets(1.0e-3), sky_bites=True)
    # -- ProjTex ---------------------------------------------------------------------------------------------------------------
    for i in (1, 3, 4, 7, 12, 13, 15):
        add("projtex_%d_denormal" % i, "clear", GENERAL, post=elem("ProjTex", i, 1.0e-45))
    add("projtex_14_above_one", "clear", GENERAL, post=elem("ProjTex", 14, up(1.0)))
    add("projtex_14_under_one", "clear", GENERAL, post=elem("ProjTex", 14, down(1.0)))
    add("projtex_1_minus_zero", "clear", {}, post=elem("ProjTex", 1, -0.0))
    add("projtex_1_sheared_cull", "cull", GENERAL, post=elem("ProjTex", 1, 0.05))
    add("projtex_13_sheared_sky", "sky", GENERAL, post=elem("ProjTex", 13, 0.01))
    add("projtex_0_under_1e12", "clear", dict(sky=0), post=elem("ProjTex", 0, down(BIG)))            # dx is far over 4096
    add("projtex_0_1e12", "clear", GENERAL, post=elem("ProjTex", 0, BIG))
    add("projtex_0_-1e12", "clear", GENERAL, post=elem("ProjTex", 0, -BIG))
    add("projtex_6_1e12", "clear", GENERAL, post=elem("ProjTex", 6, BIG))
    # -- BlurWeights -----------------------------------------------------------------------------------------------------------
    off = dict(weights=0)
    for frame in ("wall", "wallsky", "clear"):
        add("weights_reference_" + frame, frame, {}, blur=True)
        add("weights_one_zero_" + frame, frame, off, post=one_weight(0, 0.0), blur=True)
        add("weights_denormal_" + frame, frame, {}, post=weights([1.0e-45] * 11), blur=True)
    for sigma in (0.5, 1.0, 1.5, 2.0):
        add("weights_gauss_%g_padded" % sigma, "wall", off, post=gauss_padded(sigma), blur=True)
    add("weights_gauss_1.5_padded_wallsky", "wallsky", off, post=gauss_padded(1.5), blur=True)
    add("weights_min_normal", "wall", {}, post=weights([1.1754944e-38] * 11), blur=True)
    add("weights_under_1e30", "wall", {}, post=weights([down(W_MAX)] * 11), blur=True)
    add("weights_under_1e30_wallsky", "wallsky", {}, post=weights([down(W_MAX)] * 11), blur=True)
    add("weights_one_1e30", "wall", off, post=one_weight(7, W_MAX), blur=True)
    add("weights_one_minus_zero", "wall", off, post=one_weight(10, -0.0), blur=True)
    add("weights_zero_centre", "wall", off, post=one_weight(5, 0.0), blur=True)
    add("weights_one_negative", "wall", off, post=one_weight(3, -0.05), blur=True)
    add("weights_one_inf", "wall", off, post=one_weight(4, math.inf), blur=True)
    add("weights_one_nan", "wall", off, post=one_weight(6, math.nan), blur=True)
    add("weights_one_nan_wallsky", "wallsky", off, post=one_weight(6, math.nan), blur=True)
    add("weights_one_inf_wallsky", "wallsky", off, post=one_weight(4, math.inf), blur=True)
    add("weights_all_negative_wallsky", "wallsky", off, post=weights([-1.0 / 11.0] * 11), blur=True)
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


CASES = _cases()


# ---- frames ----------------------------------------------------------------------------------------------------------------------
class Frame:
    def __init__(self, W, H, c, depth, normal, randvec):
        self.W, self.H, self.c, self.depth, self.normal, self.randvec = W, H, c, depth, normal, randvec
        self.cb = c.ssao_cb


def make_constants(W, H, cam, pre=None):
    """A scene.Constants of its own for (near, far, fovY) with the edit `pre` applied."""
    from crychic_renderer_amd import scene
    camera = scene.default_camera(W, H)
    camera.nearZ, camera.farZ, camera.fovY = cam
    c = scene.Constants(W, H, shadow_dim=64, cam=camera)
    if pre is not None:
        pre(c.ssao_cb)
    return c


_planes = {}


def build_frame(case):
    """The case's frame: the planes come from fuzz_util's builder run on the case's own camera and `pre` edit (cached per frame kind,
    seed, camera and edit, and read-only); the constants are a fresh object per call, so nothing a case writes reaches another."""
    import fuzz_util
    W, H = FRAME_SIZE[case.frame]
    key = (case.frame, case.seed, case.cam, case.name if case.pre is not None else None)
    if key not in _planes:
        c = make_constants(W, H, case.cam, case.pre)
        if case.frame == "clear":
            planes = fuzz_util.clear_cell_probe_case(case.seed, consts=c)[4:]
        elif case.frame == "sky":
            planes = fuzz_util.sky_probe_case(case.seed, consts=c)[4:]
        elif case.frame == "cull":
            planes = fuzz_util.cull_probe_case(case.seed, W, H, consts=c)[3:]
        else:
            planes = fuzz_util.rough_wall_case(case.seed, W, H, case.frame == "wallsky", consts=c)[2:]
        planes = tuple(np.ascontiguousarray(p) for p in planes)
        for p in planes:
            p.flags.writeable = False
        _planes[key] = planes
    depth, normal, randvec = _planes[key]
    return Frame(W, H, case_constants(case), depth, normal, randvec)


def case_constants(case):
    """The case's constants alone (a fresh scene.Constants; its ssao_cb is the case's constant buffer)."""
    W, H = FRAME_SIZE[case.frame]
    c = make_constants(W, H, case.cam, case.pre)
    c.ssao_cb = copy.deepcopy(c.ssao_cb)
    if case.frame == "clear":
        c.ssao_cb.OcclusionRadius = 3.0 * case.cam[0]            # as fuzz_util.clear_cell_probe_case sets it
    if case.post is not None:
        case.post(c.ssao_cb)
    return c


def strips(H):
    """Two row strips of the half-res map: one at the top, one in the middle that starts off every tile boundary."""
    h2 = H // 2
    return ((0, h2 // 8), (h2 // 3 + 1, h2 // 5))


def dump_constants(path):
    """Every case's constant buffer into one binary file: a uint32 count, then the crychic_ssao_constants one after the other (what
    tests/hostsim/ssao_guards_san_main.cpp reads)."""
    with open(path, "wb") as f:
        f.write(np.uint32(len(CASES)).tobytes())
        for case in CASES:
            cb = case_constants(case).ssao_cb
            f.write(C.string_at(C.addressof(cb), C.sizeof(cb)))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dump_constants(sys.argv[1])
