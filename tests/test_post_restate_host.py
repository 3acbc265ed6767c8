"""The four depth-reading post passes held to a second reference that shares no code with the first: the C checkers (tests/*_ref)
against the float64 / int64 restatements of tests/post_restate.py, over the corpus cases of at most 128 x 96 pixels; the physical
anchor (the synthetic scene's true world points); and the mutation table.  The margins and caps are derived in DESIGN.md section 26
and recorded with the measured shares in profiles/post_restate.txt.  The judges here take any provider of a pass's outputs, so
tests/test_post_restate_gpu.py applies the same assertions to the device."""
import numpy as np
import pytest

import dof_lib as dl
import fog_lib as fg
import motion_blur_lib as mbl
import post_restate as pr
import taa_lib as tl

SMALL = 128 * 96
_CACHE = {}


def cached(key, make):
    """The unmutated restatement's result for `key`, computed once and shared by the CPU tier, the GPU tier and the mutations."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def share(n, of):
    return 100.0 * n / max(of, 1)


# ---- motion blur -----------------------------------------------------------------------------------------------------------------------

MB_STEP_CAP = 0.5           # per cent of the pixels whose step-A word may differ at all


def mb_cases():
    return [c for c in mbl.corpus() if c.W * c.H <= SMALL]


def mb_checker(case):
    ws, out, _ = mbl.expected(case)
    return ws, out


def judge_motion_blur(outputs_of, cases, mutation=None):
    """(failures, shares).  outputs_of(case) = (workspace bytes, frame)."""
    fails, px, differ, moved = [], 0, 0, 0
    for case in cases:
        ws, out = outputs_of(case)
        words, depths, tiles = mbl.velocity_words(np.asarray(ws), case.W, case.H)
        make = lambda: pr.mb_step_a64(case, mutation)
        qx, qy, ab = make() if mutation else cached(("mb", case.name), make)
        cx, cy, _ = pr.word_parts(words)
        over = ((np.abs(cx - qx) > 1) | (np.abs(cy - qy) > 1)) & ~ab
        d = (cx != qx) | (cy != qy) | ab
        n = case.W * case.H
        px, differ = px + n, differ + int(d.sum())
        if over.any():
            fails.append("%s: step A: %d words further than 1 from floor(s 16 + 0.5)" % (case.name, int(over.sum())))
        if n >= 1000 and share(int(d.sum()), n) > MB_STEP_CAP:
            fails.append("%s: step A: %.3f %% of the words differ" % (case.name, share(int(d.sum()), n)))
        if not np.array_equal(depths, case.depth & 0xFFFFFF):
            fails.append("%s: step A: the depth fields" % case.name)
        t64 = pr.mb_tiles64(words, mutation)
        f64 = pr.mb_gather64(case.img, words, depths, tiles, case.samples, mutation=mutation)
        bad = int((t64 != tiles).sum()), int((f64 != out).any(axis=-1).sum())
        moved += bad[1] + bad[0]
        if bad[0]:
            fails.append("%s: step A': %d tile words differ" % (case.name, bad[0]))
        if bad[1]:
            fails.append("%s: step B: %d pixels differ" % (case.name, bad[1]))
    if share(differ, px) > MB_STEP_CAP:
        fails.append("step A: %.3f %% of the corpus's words differ" % share(differ, px))
    return fails, dict(pixels=px, step_a_differ=differ, step_a_share=share(differ, px), back_end_differ=moved,
                       back_end_share=share(moved, px))


# ---- temporal anti-aliasing -------------------------------------------------------------------------------------------------------------

TAA_OFFSET_CAP, TAA_UNDECIDED_CAP = 1.0, 0.5        # per cent of the corpus


def taa_cases():
    return [c for c in tl.corpus() if c.W * c.H <= SMALL]


def taa_checker(case, row0=0, rows=None):
    if row0 == 0 and rows is None:
        return tl.expected(case)[:2]
    out, hout, _ = tl.checker(case, row0, rows)
    return out, hout


def _taa_compare(case, front, got, row0, rows, mutation):
    """Per pixel of the rows: (ok, needed a non-zero offset)."""
    ys = slice(row0, row0 + rows)
    out, hout = got[0][ys], got[1][ys]
    with_h, without = pr.taa_candidates64(case, front, row0, rows, mutation)
    eq = lambda pair: (pair[0] == out).all(axis=-1) & (pair[1] == hout).all(axis=-1)
    m = [eq(p) for p in with_h]
    any_h, no_h = np.any(m, axis=0), eq(without)
    has, decided = front["has"][ys], front["decided"][ys]
    ok = np.where(decided, np.where(has, any_h, no_h), any_h | no_h)
    # a pixel whose history texels equal the frame's own gives the same bytes on both branches: no offset was needed if either fits
    return ok, decided & has & any_h & ~m[0]


def judge_taa(outputs_of, cases, mutation=None, row_ranges=True, input_caps=True):
    """(failures, shares).  outputs_of(case, row0, rows) = (out, history_out), whole planes of which the rows are read.  input_caps:
    assert the caps that depend on the cases and the restatement alone, not on the outputs; they are stated for the whole corpus."""
    fails, px, offset, undecided, wrong, wrong_rows = [], 0, 0, 0, 0, 0
    for case in cases:
        make = lambda: pr.taa_front64(case, mutation)
        front = make() if mutation else cached(("taa", case.name), make)
        ok, off = _taa_compare(case, front, outputs_of(case, 0, None), 0, case.H, mutation)
        px, offset, undecided = px + case.W * case.H, offset + int(off.sum()), undecided + int((~front["decided"]).sum())
        wrong += int((~ok).sum())
        if not ok.all():
            fails.append("%s: %d pixels equal no candidate of their branch" % (case.name, int((~ok).sum())))
        if row_ranges and case.H >= 7:
            row0, rows = 2, case.H - 4
            ok, _ = _taa_compare(case, front, outputs_of(case, row0, rows), row0, rows, mutation)
            wrong_rows += int((~ok).sum())
            if not ok.all():
                fails.append("%s, rows [%d, %d): %d pixels equal no candidate" % (case.name, row0, row0 + rows, int((~ok).sum())))
    if share(offset, px) >= TAA_OFFSET_CAP:
        fails.append("%.3f %% of the pixels needed a non-zero offset" % share(offset, px))
    if input_caps and share(undecided, px) > TAA_UNDECIDED_CAP:
        fails.append("%.3f %% of the pixels are undecided" % share(undecided, px))
    return fails, dict(pixels=px, offset=offset, offset_share=share(offset, px), undecided=undecided,
                       undecided_share=share(undecided, px), wrong=wrong, wrong_share=share(wrong, px),
                       wrong_in_row_ranges=wrong_rows)


# ---- depth of field ---------------------------------------------------------------------------------------------------------------------

DOF_CLEAN_FLOOR = 95.0      # per cent of the pixels whose disc holds no marginal texel


def dof_cases():
    return [c for c in dl.corpus() if c[2].shape[0] * c[2].shape[1] <= SMALL]


def dof_checker(case, row0=0, rows=None):
    """(frame, the checker's plane of circles of confusion)."""
    name, frame, img, pname, _ = case
    if row0 == 0 and rows is None:
        coc = cached(("dof_coc", name), lambda: dl.checker(frame, img, dl.PARAM_SETS[pname], coc=True)[2])
        return dl.expected(name)[0], coc
    return dl.checker(frame, img, dl.PARAM_SETS[pname], row0, rows)[0], None


def judge_dof(outputs_of, cases, mutation=None, row_ranges=True, input_caps=True):
    """(failures, shares).  outputs_of(case, row0, rows) = (frame, the (H, W) plane of c the back end is fed, or None in a row range).
    input_caps as in judge_taa."""
    fails, texels, marginal_texels, px, clean, moved, moved_rows = [], 0, 0, 0, 0, 0, 0
    for case in cases:
        name, frame, img, pname, _ = case
        params = dl.PARAM_SETS[pname]
        R = params["radius"]
        H, W = img.shape[:2]
        out, coc = outputs_of(case, 0, None)
        c64, marginal = cached(("dof", name), lambda: pr.dof_c64(pr.dof_u64(frame, params), R))
        texels, marginal_texels = texels + H * W, marginal_texels + int(marginal.sum())
        bad = (c64 != coc) & ~marginal
        if bad.any():
            fails.append("%s: %d circles of confusion differ outside the margin" % (name, int(bad.sum())))
        back = pr.dof_back64(coc, frame.depth, img, R, mutation=mutation)
        n = int((back != out).any(axis=-1).sum())
        moved += n
        if n:
            fails.append("%s: the back end on the given c plane: %d pixels differ" % (name, n))
        whole = pr.dof_back64(c64, frame.depth, img, R, mutation=mutation)
        ok = ~pr.dof_marginal_discs(marginal, R)
        px, clean = px + H * W, clean + int(ok.sum())
        n = int(((whole != out).any(axis=-1) & ok).sum())
        if n:
            fails.append("%s: the whole restatement: %d pixels without a marginal texel differ" % (name, n))
        if row_ranges and H >= 7:
            row0, rows = 2, H - 4
            got = outputs_of(case, row0, rows)[0][row0:row0 + rows]
            n = int((pr.dof_back64(coc, frame.depth, img, R, row0, rows, mutation) != got).any(axis=-1).sum())
            moved_rows += n
            if n:
                fails.append("%s, rows [%d, %d): %d pixels differ" % (name, row0, row0 + rows, n))
    if input_caps and share(clean, px) < DOF_CLEAN_FLOOR:
        fails.append("only %.2f %% of the pixels have a disc without a marginal texel" % share(clean, px))
    return fails, dict(texels=texels, marginal_texels=marginal_texels, pixels=px, clean=clean, clean_share=share(clean, px), back_end_differ=moved,
                       back_end_share=share(moved, px), differ_in_row_ranges=moved_rows)


# ---- volumetric fog ----------------------------------------------------------------------------------------------------------------------

FOG_EXACT_FLOOR, FOG_TWO_FLOOR = 90.0, 95.0         # per cent of the channels with lo == hi, and with hi - lo <= 2


def fog_cases():
    """The corpus cases of at most 128 x 96 pixels; the ivp_* cases (non-finite InvViewProj) stay with the checker."""
    return [c for c in fg.corpus() if c[2].shape[0] * c[2].shape[1] <= SMALL and not c[0].startswith("ivp_")]


def fog_checker(case):
    return fg.expected(case[0])[0]


def judge_fog(outputs_of, cases, mutation=None, input_caps=True):
    """(failures, shares).  outputs_of(case) = the fogged frame.  input_caps as in judge_taa."""
    fails, ch, exact, two, outside, samples, marginal = [], 0, 0, 0, 0, 0, 0
    for case in cases:
        name, frame, img, pname, _ = case
        make = lambda: pr.fog64(frame, img, fg.PARAM_SETS[pname], mutation)
        lo, hi, st = make() if mutation else cached(("fog", name), make)
        out = np.asarray(outputs_of(case))
        got = out[..., :3].astype(np.int64)
        bad = (got < lo) | (got > hi)
        ch, exact, two = ch + got.size, exact + int((lo == hi).sum()), two + int((hi - lo <= 2).sum())
        samples, marginal = samples + st["samples"], marginal + st["marginal"]
        outside += int(bad.sum())
        if bad.any():
            fails.append("%s: %d channels outside [lo, hi]" % (name, int(bad.sum())))
        if not np.array_equal(out[..., 3], img[..., 3]):
            fails.append("%s: alpha" % name)
    if input_caps and share(exact, ch) < FOG_EXACT_FLOOR:
        fails.append("lo == hi on only %.2f %% of the channels" % share(exact, ch))
    if input_caps and share(two, ch) < FOG_TWO_FLOOR:
        fails.append("hi - lo <= 2 on only %.2f %% of the channels" % share(two, ch))
    return fails, dict(channels=ch, exact_share=share(exact, ch), two_share=share(two, ch), outside=outside, outside_share=share(outside, ch),
                       marginal_sample_share=share(marginal, samples))


# ---- the CPU tier: checker against restatement ---------------------------------------------------------------------------------------------

def report(title, shares):
    print("%s: %s" % (title, ", ".join("%s %s" % (k, ("%.3f" % v) if isinstance(v, float) else v) for k, v in shares.items())))


def test_motion_blur_checker_meets_the_restatement():
    """Step A within 1 of floor(s 16 + 0.5) on every word, differing on at most 0.5 % of any case of 1000 pixels or more and of the
    corpus (the nan and inf cameras included); steps A' and B from the checker's own velocity plane: every byte."""
    fails, shares = judge("motion_blur")
    report("motion blur, checker", shares)
    assert not fails, fails


def test_taa_checker_meets_the_restatement():
    """Decided pixels equal the integer back end at the float64 history position or a neighbour of it (fewer than 1 % need one);
    undecided pixels (at most 0.5 %) equal a candidate of either branch; whole frames and the row range [2, H - 2)."""
    fails, shares = judge("taa")
    report("temporal anti-aliasing, checker", shares)
    assert not fails, fails


def test_dof_checker_meets_the_restatement():
    """c64 == c outside the margin; the back end on the checker's c plane: every pixel; the whole restatement: every pixel whose disc
    holds no marginal texel, at least 95 % of the corpus; whole frames and the row range [2, H - 2)."""
    fails, shares = judge("dof")
    report("depth of field, checker", shares)
    assert not fails, fails


def test_fog_checker_lies_in_the_restatements_interval():
    """Every R, G, B byte in [lo, hi]; lo == hi on at least 90 % and hi - lo <= 2 on at least 95 % of the channels.  The ivp_* cases
    are left to the checker."""
    fails, shares = judge("fog")
    report("fog, checker", shares)
    assert not fails, fails


# ---- the physical anchor -------------------------------------------------------------------------------------------------------------------

ANCHOR_SIZES = ((128, 96), (70, 38))
ANCHOR_CAMERAS = {"strafe": dict(dx=0.35), "yaw": dict(yaw=0.12), "dolly": dict(dz=-1.5), "mix": dict(dx=0.5, dz=0.8, yaw=0.12)}
ANCHOR_SLACK = 1.0 / 64.0       # of a 1/16 pixel (motion blur) or of a 1/256 texel (TAA): the depth step and binary32
_ANCHOR = {}


def anchor_scene(W, H, jitter=(0.0, 0.0)):
    """The synthetic scene's camera planes: dict of depth (H, W) uint32, true (H, W, 3) float64 world points (the ray-caster's, rounded
    to binary32 in g0), covered, ivp (of the frame's own constants), cur (the unjittered view-projection), eye, look, A, B."""
    key = (W, H, jitter)
    if key not in _ANCHOR:
        from crychic_renderer_amd import scene
        consts = scene.Constants(W, H, shadow_dim=64, jitter=jitter)
        planes = scene._camera_planes(consts, "cpu")
        depth = np.ascontiguousarray(planes["depth"].numpy().view(np.uint32))
        _ANCHOR[key] = dict(depth=depth, true=planes["g0"].numpy()[..., :3].astype(np.float64), covered=(depth & 0xFFFFFF) < 0xFFFFFF,
                            ivp=np.array(consts.pass_cb.InvViewProj[:], np.float32), cur=tl.camera_matrices(W, H)[0],
                            eye=np.array(consts.cam.pos[:], np.float64), look=np.array(consts.cam.look[:], np.float64),
                            A=float(consts.pass_cb.Proj[10]), B=float(consts.pass_cb.Proj[11]))
    return _ANCHOR[key]


def anchor_motion_blur_case(W, H, camera):
    """The scene's depth plane under a moved previous camera, the shutter open for the whole frame interval and R = 32."""
    s = anchor_scene(W, H)
    prev = tl.camera_matrices(W, H, cam=tl.moved_camera(W, H, **ANCHOR_CAMERAS[camera]))[0]
    img = np.random.default_rng(26).integers(0, 256, (H, W, 4), dtype=np.uint8)
    return mbl.Case("anchor_%dx%d_%s" % (W, H, camera), s["ivp"], s["cur"], prev, s["depth"], img, shutter=256, samples=8, radius=32)


def anchor_taa_case(W, H, camera, jitter=(0.25, -0.375)):
    """The scene's depth plane of a jittered frame over a history whose R and G hold 256 x and 256 y: with a black frame, blend 1 and
    NO_CLAMP, history_out holds (255 X + 128) >> 8 and (255 Y + 128) >> 8 of the integer history position (X, Y)."""
    s = anchor_scene(W, H, jitter)
    prev = tl.camera_matrices(W, H, cam=tl.moved_camera(W, H, **ANCHOR_CAMERAS[camera]))[0]
    hist = np.zeros((H, W, 4), np.uint16)
    hist[..., 0], hist[..., 1] = 256 * np.arange(W)[None, :], 256 * np.arange(H)[:, None]
    return tl.Case("anchor_%dx%d_%s" % (W, H, camera), s["ivp"], s["cur"], prev, s["depth"], np.zeros((H, W, 4), np.uint8), hist, blend=1,
                   flags=tl.NO_CLAMP)


def true_velocity(s, case):
    """The velocity in pixels of the scene's true points between the case's two view-projections, and their (a3, b3)."""
    v = pr.velocity64(None, case.cur, case.prev, None, case.W, case.H, P=s["true"])
    return v["vx"], v["vy"], v["a3"], v["b3"]


@pytest.mark.parametrize("W,H", ANCHOR_SIZES)
def test_anchor_world_point(W, H):
    """(a) world_point64 lies within the D24 half-step of the ray-caster's point on every covered pixel.  With view depth
    z = B / (d - A), a step of 2^-25 in d moves the point by z^2 / (|B| 2^25) along the view axis, |r| / z times that along the ray;
    h.w = d m[2] + m[3] cancels to 1 / z from two binary32 entries of magnitude about 1 / |B|, each allowed 1.5 ulp: three more such
    steps; and g0 holds the true point rounded to binary32, 2^-24 of its largest coordinate (2^-22 bounds the three components and
    the eye)."""
    s = anchor_scene(W, H)
    P = pr.world_point64(s["ivp"], s["depth"], W, H)
    r = s["true"] - s["eye"]
    z, rl = r @ s["look"], np.linalg.norm(r, axis=-1)
    bound = 4.0 * z * rl / (abs(s["B"]) * 2.0 ** 25) + 2.0 ** -22 * (1.0 + np.abs(s["true"]).max(axis=-1))
    err = np.linalg.norm(P - s["true"], axis=-1)[s["covered"]]
    print("world point, %d x %d: max %.3g, median %.3g world units over %d covered pixels; largest share of the bound %.3f" %
          (W, H, err.max(), np.median(err), err.size, (err / bound[s["covered"]]).max()))
    assert s["covered"].sum() > W * H // 4
    assert (err <= bound[s["covered"]]).all()


@pytest.mark.parametrize("camera", list(ANCHOR_CAMERAS))
@pytest.mark.parametrize("W,H", ANCHOR_SIZES)
def test_anchor_motion_blur_velocity(W, H, camera):
    """(b) the checker's quantised word lies within 0.5 + 1/64 of a 1/16 pixel of the velocity of the true points."""
    s, case = anchor_scene(W, H), anchor_motion_blur_case(W, H, camera)
    words = mbl.velocity_words(mbl.expected(case)[0], W, H)[0]
    worst = anchor_velocity_excess(s, case, words)
    print("motion blur velocity, %s: the largest distance from the true velocity is %.5f of a 1/16 pixel" % (case.name, worst))
    assert worst <= 0.5 + ANCHOR_SLACK


def anchor_velocity_excess(s, case, words):
    vx, vy, a3, b3 = true_velocity(s, case)
    sx16, sy16, valid = pr.mb_scale64(vx, vy, a3, b3, case.shutter, case.radius)
    cov = s["covered"]
    assert valid[cov].all()         # the Chebyshev clamp to R is applied to the true velocity as the header applies it
    qx, qy, _ = pr.word_parts(words)
    return float(np.maximum(np.abs(qx - sx16), np.abs(qy - sy16))[cov].max())


@pytest.mark.parametrize("camera", list(ANCHOR_CAMERAS))
@pytest.mark.parametrize("W,H", ANCHOR_SIZES)
def test_anchor_taa_history_position(W, H, camera):
    """(c) the checker's integer history position lies within 1/256 texel, plus 1/64 of one, of where the true point was in the
    previous frame: X <= fxp < X + 1.  The position is read back through a history of coordinates; (255 X + 128) >> 8 leaves at most
    two candidates X, of which one must fit."""
    case = anchor_taa_case(W, H, camera)
    n, worst = anchor_history_excess(anchor_scene(W, H, (0.25, -0.375)), case, tl.expected(case)[1])
    print("TAA history position, %s: %d pixels, the largest excess over the 1/256 texel is %.5f of one" % (case.name, n, worst))
    assert n > W * H // 4
    assert worst <= ANCHOR_SLACK


def anchor_history_excess(s, case, hout):
    """(pixels tested, the largest distance in 1/256 texel by which the true history position misses [X, X + 1) for the best
    candidate X)."""
    W, H = case.W, case.H
    vx, vy, _, b3 = true_velocity(s, case)
    fxp, fyp = (np.arange(W)[None, :] - vx) * 256.0, (np.arange(H)[:, None] - vy) * 256.0
    # the true position at least a texel inside the frame: the pixel has history and no bilinear tap is clamped
    inner = s["covered"] & (b3 > 0) & (fxp >= 256) & (fxp <= (W - 2) * 256.0) & (fyp >= 256) & (fyp <= (H - 2) * 256.0)
    worst = 0.0
    for ch, f in ((0, fxp), (1, fyp)):
        n = hout[..., ch].astype(np.int64)
        x_lo, x_hi = -((128 - 256 * n) // 255), (256 * n + 127) // 255       # the integers X with (255 X + 128) >> 8 == n
        miss = np.maximum(np.maximum(x_lo - f, f - (x_hi + 1)), 0.0)
        worst = max(worst, float(miss[inner].max()))
    return int(inner.sum()), worst


# ---- long and thin frames ------------------------------------------------------------------------------------------------------------------

# the smallest shapes past 65535 columns or rows, at which a 16-bit coordinate can go wrong, and two either side of 4096; about
# 131 000 pixels each
THIN_SIZES = ((4100, 3), (3, 4100), (65600, 2), (2, 65600))
_THIN = {}


def thin_case(pass_name, W, H):
    """Random planes under the reference camera and a moved one: a Case of motion_blur_lib or taa_lib, or (frame, image, parameters)
    of dof_lib or fog_lib, with what the checker makes of it; built once, read-only."""
    key = (pass_name, W, H)
    if key in _THIN:
        return _THIN[key]
    rng = np.random.default_rng([26, W, H])
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    depth = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32)
    moved = tl.moved_camera(W, H, dx=0.35, dz=-0.5, yaw=0.02)
    if pass_name in ("motion_blur", "taa"):
        cur, ivp = tl.camera_matrices(W, H)
        prev = tl.camera_matrices(W, H, cam=moved)[0]
        if pass_name == "motion_blur":
            case = mbl.Case("thin_%dx%d" % (W, H), ivp, cur, prev, depth, img)
            ws, _ = mbl.checker_velocity(case)
            want = (ws, mbl.checker_gather(case, ws))
        else:
            case = tl.Case("thin_%dx%d" % (W, H), ivp, cur, prev, depth, img, tl.make_history("random", img, rng))
            want = tl.checker(case)[:2]
    elif pass_name == "dof":
        case = (dl.Frame(dl.REFERENCE_AB, depth), img, dl.DEFAULTS)
        want = dl.checker(*case)[0]
    else:
        frame = fg.Frame.from_pass_cb(fg.camera_constants(W, H, 17, cam=moved), depth, fg.make_maps("random", 17, rng))
        case = (frame, img, fg.DEFAULTS)
        want = fg.checker(*case)[0]
    _THIN[key] = (case, want)
    return _THIN[key]


@pytest.mark.parametrize("W,H", THIN_SIZES)
def test_long_thin_frames_host_bodies_equal_the_checkers(W, H):
    """The host builds of the four kernel bodies over the long and thin frames, byte for byte: the workgroup walk and the addressing
    are the kernels' own, so an index that overflows shows here before it can write out of bounds on a device."""
    import dof_host_lib
    import fog_host_lib
    import motion_blur_host_lib
    import taa_host_lib
    case, want = thin_case("motion_blur", W, H)
    ws, _ = motion_blur_host_lib.velocity(case)
    assert np.array_equal(ws, want[0]) and np.array_equal(motion_blur_host_lib.gather(case, ws)[0], want[1])
    case, want = thin_case("taa", W, H)
    out, hout, _ = taa_host_lib.taa(case)
    assert np.array_equal(out, want[0]) and np.array_equal(hout, want[1])
    (frame, img, params), want = thin_case("dof", W, H)
    raw, out = dl.guarded(img.shape)
    dof_host_lib.dof(frame, img, out, params)
    assert np.array_equal(out, want) and dl.guards_intact(raw, out)
    (frame, img, params), want = thin_case("fog", W, H)
    raw, out = fg.guarded(img.shape)
    fog_host_lib.fog(frame, img, out, params)
    assert np.array_equal(out, want) and fg.guards_intact(raw, out)


# ---- the mutations ---------------------------------------------------------------------------------------------------------------------

# Listed in the issue and not killed, with the reason:
#   motion blur, d24_pow2   a relative change of 2^-24 in d, as large as one binary32 rounding: below 2^-14 of a 1/16 pixel at any R
#   taa, b3_ge              b[3] == 0 makes rcp(b[3]) infinite: fxp is infinite or NaN and fails the bounds: equivalent on every input
#   dof, ds_ge_dp           D_s == D_p means equal depth words, so c_s == c_p and min(c_s, c_p) == c_s: equivalent on every input
#   fog, cascade_le         } differ only where the two float64 operands are equal, which is inside the margin by construction: the
#   fog, sz_lt_map          } sample is marginal either way and the interval is the same
SURVIVORS = (("motion_blur", "d24_pow2"), ("taa", "b3_ge"), ("dof", "ds_ge_dp"), ("fog", "cascade_le"), ("fog", "sz_lt_map"))
BITES = [b for b in [("motion_blur", m) for m in pr.MUTATIONS["front"] + pr.MUTATIONS["motion_blur"]] +
         [("taa", m) for m in pr.MUTATIONS["front"] + pr.MUTATIONS["taa"]] + [("dof", m) for m in pr.MUTATIONS["dof"]] +
         [("fog", m) for m in pr.MUTATIONS["front"] + pr.MUTATIONS["fog"]] if b not in SURVIVORS]


def judge(pass_name, mutation=None):
    if mutation is None:
        return cached(("judge", pass_name), lambda: judge(pass_name, ""))
    mutation = mutation or None
    return {"motion_blur": lambda: judge_motion_blur(mb_checker, mb_cases(), mutation),
            "taa": lambda: judge_taa(taa_checker, taa_cases(), mutation),
            "dof": lambda: judge_dof(dof_checker, dof_cases(), mutation),
            "fog": lambda: judge_fog(fog_checker, fog_cases(), mutation)}[pass_name]()


@pytest.mark.parametrize("pass_name,mutation", BITES)
def test_restatement_bites(pass_name, mutation):
    """One misreading of the header made on purpose in the restatement: that pass's comparison with the checker must fail on the
    corpus.  fog's t_round_32767 is killed by the case added for it, 64x64_t_rounding_tie_default, and by no other."""
    fails, shares = judge(pass_name, mutation)
    report("%s with %s: %d assertions fail, the first: %s" % (pass_name, mutation, len(fails), fails[:1]), shares)
    assert fails, "the corpus cannot tell %s from the header's text" % mutation
    if mutation == "t_round_32767":
        assert all(f.startswith("64x64_t_rounding_tie_default") for f in fails), fails


@pytest.mark.parametrize("pass_name,mutation", SURVIVORS)
def test_mutations_the_comparison_cannot_see(pass_name, mutation):
    """Recorded, not killed: the reasons stand above SURVIVORS.  The day one of them is seen, it belongs in BITES."""
    fails, shares = judge(pass_name, mutation)
    report("%s with %s" % (pass_name, mutation), shares)
    assert not fails
    if mutation != "d24_pow2":
        assert shares == judge(pass_name)[1]
