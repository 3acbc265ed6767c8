"""crychic_motion_blur on the CPU tier: the kernel bodies (csrc/motion_blur_core.hpp, built for the host with the workgroup and lane
walk emulated) against the checker (tests/motion_blur_ref, plain C from the definition in include/crychic_hip.h), byte for byte on the
workspace and the frame over the whole corpus, behind guard bytes and on misaligned planes; what the corpus must reach, on the
checker's branch masks; the definition's known answers with values worked out by hand; row ranges; and the refusals of the real
library, which need no device."""
import ctypes as C

import numpy as np
import pytest

import motion_blur_host_lib as host
import motion_blur_lib as mbl


@pytest.fixture(scope="module")
def cases(built_lib):
    return mbl.corpus()


def run_host(case, row0=0, rows=None, misalign=0, ws_in=None, img=None):
    """The kernel bodies on guarded copies of the case's planes, `misalign` bytes past a 16-byte boundary (8 at the most for the
    workspace): (workspace, out); the velocity body runs unless `ws_in` is given; asserts the guard bytes around every plane and that
    no input changed."""
    H, W = case.H, case.W
    frame = case.img if img is None else np.ascontiguousarray(img, np.uint8)
    sraw, src = mbl.guarded(frame.shape, misalign=misalign)
    draw, depth = mbl.guarded(case.depth.shape, np.uint32, misalign=misalign)
    oraw, out = mbl.guarded(frame.shape, misalign=misalign)
    wraw, ws = mbl.guarded((mbl.workspace_bytes(W, H),), misalign=misalign & 8)
    src[...] = frame
    depth[...] = case.depth
    c = mbl.Case(case.name, case.ivp, case.cur, case.prev, depth, src, case.shutter, case.samples, case.radius)
    c.img, c.depth = src, depth                       # the guarded planes themselves, not copies
    if ws_in is None:
        host.velocity(c, ws)
    else:
        ws[...] = ws_in
    before = ws.copy()
    host.gather(c, ws, row0, rows, out)
    for raw, view in ((sraw, src), (draw, depth), (oraw, out), (wraw, ws)):
        assert mbl.guards_intact(raw, view), "guard bytes changed"
    assert np.array_equal(src, frame) and np.array_equal(depth, case.depth) and np.array_equal(ws, before), "an input plane changed"
    return ws.copy(), out.copy()


def test_the_layout_functions_agree(built_lib):
    lib = built_lib.lib
    for W, H in mbl.SIZES + ((3840, 2160), (1 << 14, 1 << 14)):
        assert lib.crychic_motion_blur_tile_offset(W, H) == mbl.tile_offset(W, H)
        assert lib.crychic_motion_blur_workspace_bytes(W, H) == mbl.workspace_bytes(W, H) == host.workspace_bytes(W, H)
    assert mbl.workspace_bytes(17, 1) == 17 * 8 + 2 * 4 and mbl.workspace_bytes(70, 38) == 70 * 38 * 8 + 5 * 3 * 4


def test_host_body_equals_checker(cases):
    for case in cases:
        ref_ws, ref_out, _ = mbl.expected(case)
        for misalign in (0, 4, 12):
            ws, out = run_host(case, misalign=misalign)
            assert np.array_equal(ws, ref_ws), "%s (+%d): %d bytes of the workspace differ" % (case.name, misalign, int((ws != ref_ws).sum()))
            assert np.array_equal(out, ref_out), "%s (+%d): %d bytes of out differ" % (case.name, misalign, int((out != ref_out).sum()))
    assert len(cases) >= len(mbl.SIZES) * len(mbl.CAMERAS)


def test_the_corpus_reaches_what_it_must(cases):
    """On the checker's branch masks alone: every branch of the definition in at least 64 pixels, one case at least that blurs more than
    half its pixels, and every size, camera and parameter value the corpus promises."""
    count = dict.fromkeys(mbl.BRANCHES, 0)
    most = 0.0
    for case in cases:
        branch = mbl.expected(case)[2]
        for name, bit in mbl.BRANCHES.items():
            count[name] += int(((branch & bit) != 0).sum())
        most = max(most, float(((branch & mbl.B_STILL) == 0).mean()))
    assert all(n >= 64 for n in count.values()), count
    assert most > 0.5, most
    # a moving tile next to the frame's edge: samples clamp to the frame there
    assert any(((mbl.expected(c)[2] & mbl.B_STILL) == 0).any() and c.W % mbl.TILE and c.H % mbl.TILE for c in cases)
    for W, H in mbl.SIZES:
        at = [c for c in cases if (c.W, c.H) == (W, H)]
        assert {c.samples for c in at} >= set(mbl.SAMPLES) and {c.radius for c in at} >= set(mbl.RADII) and {c.shutter for c in at} >= set(mbl.SHUTTERS), (W, H)
        assert all(any(c.name.startswith("%dx%d_%s_" % (W, H, cam)) for c in at) for cam in mbl.CAMERAS), (W, H)


# ---- known answers --------------------------------------------------------------------------------------------------------------------

BAYER = ((0, 8, 2, 10), (12, 4, 14, 6), (3, 11, 1, 9), (15, 7, 13, 5))


def edge_case():
    """A 64 x 32 frame, black left of x = 32 and white from there on, one depth, every pixel moving 16 pixels to the left in a frame:
    shutter 256 and R = 16 leave it at that, so every velocity word is (-256, 0) and N = 8 samples span 16 pixels."""
    rng = np.random.default_rng(7)
    W, H = 64, 32
    img = np.zeros((H, W, 4), np.uint8)
    img[:, 32:, :3] = 255
    img[..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    ivp, cur, prev = mbl.translate_matrices(16.0, 0.0, W, H)
    return mbl.Case("edge", ivp, cur, prev, np.full((H, W), 0x123456, np.uint32), img, 256, 8, 16)


def foreground_case(sign=1.0):
    """48 x 48: a background at depth 1 that a shear moves 6 pixels a frame, and a 20 x 20 block at depth 0 that stands still."""
    rng = np.random.default_rng(8)
    W = H = 48
    depth = np.full((H, W), 0xFFFFFF, np.uint32)
    depth[14:34, 14:34] = 0
    ivp, cur, prev = mbl.shear_matrices(sign * 0.25, 0.0)
    return mbl.Case("foreground", ivp, cur, prev, depth, rng.integers(0, 256, (H, W, 4), dtype=np.uint8), 256, 16, 16)


def tie_case(sy):
    """16 x 16, one tile: every pixel moves 2 pixels to the left; the one at (5, 9) has depth 1 and moves 8 sy pixels vertically too."""
    rng = np.random.default_rng(9)
    depth = np.zeros((16, 16), np.uint32)
    depth[9, 5] = 0xFFFFFF
    prev = mbl.IDENTITY.copy()
    prev[3], prev[6] = 2.0 * 2.0 / 16.0, sy
    return mbl.Case("tie", mbl.IDENTITY, mbl.IDENTITY, prev, depth, rng.integers(0, 256, (16, 16, 4), dtype=np.uint8), 256, 8, 16)


def answers(run):
    """run(case) -> (workspace bytes, out)."""
    # 1. a vertical edge under a uniform translation becomes the ramp of the definition
    case = edge_case()
    ws, out = run(case)
    words, depths, tiles = mbl.velocity_words(ws, case.W, case.H)
    assert (words == mbl.word(-256, 0)).all() and (depths == 0x123456).all() and (tiles == mbl.word(-256, 0)).all()
    # by hand, rows with py & 3 == 0 and columns with px & 3 == 0 (b = 0): m = 16 i - 64, ox = floor((-256 m + 64) / 128) = -2 m =
    # 128, 96, 64, 32, 0, -32, -64, -96, pixel offsets (ox + 8) >> 4 = 8, 6, 4, 2, 0, -2, -4, -6; every weight is 2 (one depth, and
    # 2 dist <= 256), Wt = 17; with k white samples S = 255 (2 k + [own white]) and out = floor((2 S + 17) / 34)
    for px, value in ((16, 0), (20, 0), (24, 30), (28, 90), (32, 165), (36, 225), (40, 255), (44, 255)):
        assert (out[0::4, px, :3] == value).all(), (px, out[0, px])
    # every pixel, from the definition restated with Python's integers
    for py in range(case.H):
        for px in range(case.W):
            b = BAYER[py & 3][px & 3]
            S = int(case.img[py, px, 0])
            for i in range(8):
                ox = (-256 * (16 * i + b - 64) + 64) // 128
                S += 2 * int(case.img[py, min(max(px + ((ox + 8) >> 4), 0), case.W - 1), 0])
            assert tuple(out[py, px]) == ((2 * S + 17) // 34,) * 3 + (case.img[py, px, 3],), (px, py)
    # 2. a static foreground in front of a moving background keeps its bytes, whichever way the background moves
    for sign in (1.0, -1.0):
        case = foreground_case(sign)
        ws, out = run(case)
        words, _, tiles = mbl.velocity_words(ws, case.W, case.H)
        moving = mbl.word(int(-sign * 96), 0)
        assert (words[14:34, 14:34] == 0).all() and (words[0, :] == moving).all()
        assert tiles[1, 1] == 0 and (np.delete(tiles.reshape(-1), 4) == moving).all(), "the middle tile lies inside the block"
        assert np.array_equal(out[14:34, 14:34], case.img[14:34, 14:34])
        assert (out[:, :8] != case.img[:, :8]).any(), "the background is blurred"
    # 3. a still camera, shutter 0 and a first frame copy the frame and leave a tile plane of zeros
    rng = np.random.default_rng(10)
    W, H = 70, 38
    img, depth = rng.integers(0, 256, (H, W, 4), dtype=np.uint8), mbl.make_depth("random", W, H, rng)
    ivp, cur, moved = mbl.camera_motion("yaw", W, H)
    for name, prev, shutter in (("still", cur.copy(), 256), ("first_frame", cur, 128), ("shutter0", moved, 0)):
        case = mbl.Case(name, ivp, cur, prev, depth, img, shutter, 8, 16)
        ws, out = run(case)
        words, depths, tiles = mbl.velocity_words(ws, W, H)
        assert (words == 0).all() and (tiles == 0).all() and np.array_equal(depths, depth & 0xFFFFFF), name
        assert np.array_equal(out, img), name
    assert (run(mbl.Case("moving", ivp, cur, moved, depth, img, 256, 8, 16))[1] != img).any()
    # 4. velocities of equal length in one tile resolve to the larger word: (-32, 16) and (-32, -16) both beat (-32, 0)
    for sy, q in ((0.125, 16), (-0.125, -16)):
        case = tie_case(sy)
        words, _, tiles = mbl.velocity_words(run(case)[0], 16, 16)
        assert words[9, 5] == mbl.word(-32, q) and (np.delete(words.reshape(-1), 9 * 16 + 5) == mbl.word(-32, 0)).all()
        assert tiles.shape == (1, 1) and tiles[0, 0] == mbl.word(-32, q) > mbl.word(-32, 0)


def checker_run(case):
    ws, _ = mbl.checker_velocity(case)
    return ws, mbl.checker_gather(case, ws)


def test_known_answers(built_lib):
    answers(checker_run)
    answers(run_host)
    answers(lambda c: run_host(c, misalign=12))


# ---- row ranges -----------------------------------------------------------------------------------------------------------------------

def tall_case(camera):
    rng = np.random.default_rng(190)
    W, H = 45, 190
    ivp, cur, prev = mbl.camera_motion(camera, W, H)
    return mbl.Case("tall_" + camera, ivp, cur, prev, mbl.make_depth("ramp", W, H, rng), rng.integers(0, 256, (H, W, 4), dtype=np.uint8), 256, 8, 16)


SPLITS = [(0, 1, 2, 33, 34, 69, 190), (0, 16, 190), (0, 7, 12, 95, 189, 190)]


@pytest.mark.parametrize("split", SPLITS)
def test_row_ranges_stitch_to_the_whole_frame(built_lib, split):
    for camera in ("yaw", "dolly"):
        case = tall_case(camera)
        whole_ws, whole_out = checker_run(case)
        assert (whole_out != case.img).any()
        stitched = np.full_like(whole_out, mbl.GUARD)
        for row0, end in zip(split[:-1], split[1:]):
            ws, out = run_host(case, row0=row0, rows=end - row0)
            assert np.array_equal(ws, whole_ws), "the velocity launch covers the whole frame whatever the rows"
            assert np.array_equal(out, mbl.checker_gather(case, whole_ws, row0, end - row0)), (camera, row0, end)
            assert (out[:row0] == mbl.GUARD).all() and (out[end:] == mbl.GUARD).all(), "rows outside the range were written"
            stitched[row0:end] = out[row0:end]
        assert np.array_equal(stitched, whole_out), camera
    assert (run_host(case, row0=190, rows=0)[1] == mbl.GUARD).all() and (run_host(case, row0=17, rows=0)[1] == mbl.GUARD).all()


def test_default_params(built_lib):
    p = built_lib.MotionBlurParams()
    assert C.sizeof(p) == 32 and built_lib.lib.crychic_motion_blur_default_params(C.byref(p)) == 0
    assert (p.shutter, p.samples, p.maxRadius, p.flags, tuple(p.reserved)) == (128, 8, 16, 0, (0,) * 4)
    assert (mbl.DEFAULT_SHUTTER, mbl.DEFAULT_SAMPLES, mbl.DEFAULT_RADIUS) == (128, 8, 16)
    assert built_lib.lib.crychic_motion_blur_default_params(None) == -1
    q = built_lib.MotionBlurParams.default(shutter=256, samples=32, maxRadius=1)
    assert (q.shutter, q.samples, q.maxRadius, q.flags) == (256, 32, 1, 0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_need_no_device(built_lib):
    """Every argument is checked before the context is looked at: with a NULL context a bad argument is reported as itself, and a
    valid call gets as far as the context."""
    lib, P = built_lib.lib, built_lib.MotionBlurParams
    W, H = 64, 32
    a, b, d, w = 0x10000000, 0x20000000, 0x30000000, 0x40000000           # never dereferenced
    fb, wb = W * H * 4, mbl.workspace_bytes(W, H)
    good = built_lib.PassConstants()
    good.InvViewProj[:] = list(mbl.IDENTITY)
    eye = (C.c_float * 16)(*mbl.IDENTITY)
    wild = (C.c_float * 16)(*([float("nan"), float("inf")] * 8))
    err = lambda: lib.crychic_last_error().decode()

    def both(cb=good, cur=eye, prev=eye, depth=d, src=a, dst=b, W=W, H=H, params=None, ws=w, size=None):
        rc = lib.crychic_motion_blur(None, None if cb is None else C.byref(cb), cur, prev, depth, src, dst, W, H, None if params is None else C.byref(params), ws,
                                     mbl.workspace_bytes(W, H) if size is None else size, None)
        return rc, err()

    def velocity(cb=good, cur=eye, prev=eye, depth=d, W=W, H=H, params=None, ws=w, size=None):
        rc = lib.crychic_motion_blur_velocity(None, None if cb is None else C.byref(cb), cur, prev, depth, W, H, None if params is None else C.byref(params), ws,
                                              mbl.workspace_bytes(W, H) if size is None else size, None)
        return rc, err()

    def gather(src=a, dst=b, W=W, H=H, row0=0, rows=H, params=None, ws=w, size=None):
        rc = lib.crychic_motion_blur_gather(None, src, dst, W, H, row0, rows, None if params is None else C.byref(params), ws,
                                            mbl.workspace_bytes(W, H) if size is None else size, None)
        return rc, err()

    ok = (-1, "null context")
    assert both() == ok and velocity() == ok and gather() == ok
    assert both(cur=wild, prev=wild) == ok and velocity(prev=wild) == ok, "the matrices may hold anything"
    assert both(dst=a + fb, ws=a + 2 * fb) == ok and both(ws=a - wb) == ok and velocity(ws=d + fb) == ok, "adjacent planes do not overlap"
    assert gather(row0=H, rows=0) == ok and gather(row0=5, rows=9) == ok and both(W=1, H=1) == ok and both(size=wb + 100) == ok
    assert both(src=a + 4, dst=b + 12, depth=d + 4, ws=w + 8) == ok
    for n in mbl.SAMPLES:
        assert both(params=P.default(samples=n, shutter=0, maxRadius=1)) == ok and gather(params=P.default(samples=n, shutter=256, maxRadius=32)) == ok
    bad_res = P.default()
    bad_res.reserved[3] = 1
    params = [(dict(params=P.default(shutter=257)), "shutter"), (dict(params=P.default(samples=0)), "samples"), (dict(params=P.default(samples=1)), "samples"),
              (dict(params=P.default(samples=12)), "samples"), (dict(params=P.default(samples=64)), "samples"), (dict(params=P.default(maxRadius=0)), "maxRadius"),
              (dict(params=P.default(maxRadius=33)), "maxRadius"), (dict(params=P.default(flags=1)), "flags"), (dict(params=bad_res), "reserved"),
              (dict(ws=None), "null argument"), (dict(ws=w + 4), "8-byte aligned"), (dict(W=0), "non-zero"), (dict(H=0), "non-zero"),
              (dict(size=wb - 1), "workspace has"), (dict(size=0), "workspace has")]
    for call, more in ((both, [(dict(cb=None), "null argument"), (dict(cur=None), "null argument"), (dict(prev=None), "null argument"),
                               (dict(depth=None), "null argument"), (dict(src=None), "null argument"), (dict(dst=None), "null argument"),
                               (dict(src=a + 2), "4-byte aligned"), (dict(dst=b + 1), "4-byte aligned"), (dict(depth=d + 2), "4-byte aligned"),
                               (dict(dst=a), "cannot run in place"), (dict(dst=a + 4), "cannot run in place"), (dict(src=b + fb - 4), "cannot run in place"),
                               (dict(ws=a + fb - 8), "workspace overlaps"), (dict(ws=b - wb + 8), "workspace overlaps"), (dict(ws=d), "workspace overlaps")]),
                       (velocity, [(dict(cb=None), "null argument"), (dict(cur=None), "null argument"), (dict(prev=None), "null argument"),
                                   (dict(depth=None), "null argument"), (dict(depth=d + 1), "4-byte aligned"), (dict(ws=d + fb - 8), "workspace overlaps")]),
                       (gather, [(dict(src=None), "null argument"), (dict(dst=None), "null argument"), (dict(src=a + 2), "4-byte aligned"),
                                 (dict(dst=a), "cannot run in place"), (dict(dst=a + fb - 4), "cannot run in place"), (dict(ws=b + 8), "workspace overlaps"),
                                 (dict(row0=H + 1, rows=0), "outside the 32-row frame"), (dict(row0=1, rows=H), "outside the 32-row frame"),
                                 (dict(row0=0xFFFFFFFF, rows=2), "outside the 32-row frame")])):
        for kw, word in params + more:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (call.__name__, kw, rc, msg)
    for call in (both, velocity):
        rc, msg = call(W=1 << 15, H=(1 << 13) + 1)
        assert rc == -4 and "exceeds" in msg
        rc, msg = call(W=(1 << 22) + 1, H=1)
        assert rc == -4 and "2^22" in msg
        assert call(W=1 << 22, H=1) == ok
    rc, msg = gather(W=(1 << 22) + 1, H=1, rows=1)
    assert rc == -4 and "2^22" in msg
