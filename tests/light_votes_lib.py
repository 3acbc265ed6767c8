"""The wave votes of the lighting kernels (csrc/light_core.hpp, csrc/light_tiles.hpp) sorted on the CPU, and the frames that drive
each of them across its boundary (TEST HARNESS ONLY): builds and loads tests/hostsim/liblight_votes_host.so -- the per-lane
predicates behind the votes, compiled for the host -- groups the pixels of a call into wavefronts exactly as light_tile_pixel does,
and says of every (wavefront, vote) whether the vote is unanimous, refused or carried by exactly one lane, mixed, or not taken.

A vote is reached by a wavefront only on the path the votes before it chose (the packed cascade lookup exists only where vote 10 is
unanimous, its rim only where vote 11 is not ...): wave_votes() follows light_pixel's own order.  A vote taken more than once per
pixel -- once per cascade, once per lookup -- is one SUB-VOTE per occasion; the census pools a vote's sub-votes.

Every bit is stated in the sense in which unanimity takes the shortcut.  For vote 9 that is "the lane does NOT need cascade k":
the wavefront skips cascade k when no lane needs it.

Used by tests/test_light_votes_host.py (grouping, census, host bodies == reference) and tests/test_light_votes_gpu.py (device ==
reference); the reference is the oracle, and the family's checker for the point-shadow and the general family (CONFIGS)."""
import ctypes as C
import os

import numpy as np

import hostsim_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "light_votes_host.cpp")
LIB = os.path.join(ROOT, "tests", "hostsim", "liblight_votes_host.so")
CENSUS_FILE = os.path.join(ROOT, "profiles", "light_votes_census.txt")

FIELDS = ("COVERED", "J", "BLEND", "NEEDS", "P10", "P11", "P12", "P1A", "P1B", "P2_0", "P2_1", "P2_2", "P2_3", "P3_0", "P3_1", "P3_2",
          "P3_3", "P8", "P4", "P5", "P6", "P7")
F = {n: k for k, n in enumerate(FIELDS)}

SKY, FIX_Q1 = 1, 0x100
GLOSS, AMBIENT_SH, ENV_BRDF = 0x800, 0x8000, 0x100000          # CRYCHIC_LIGHT_CUBE_GLOSS, _AMBIENT_SH, _ENV_BRDF
HALF_G1_G2 = 0x2000 | 0x4000                    # CRYCHIC_GBUFFER_G1_F16 | G2_F16
W, H = 200, 64
SHADOW_DIM, CUBE_DIM, CUBE_LEVELS = 64, 16, 5
ROW_RANGES = ((0, H), (0, 22), (22, 20), (42, 22))


def build():
    return hostsim_lib.build_host(LIB, SRC, ())


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.lv_field_count.restype = C.c_uint32
        _LIB.lv_classify.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p] + [C.c_uint32] * 5 + [C.c_int, C.c_float, C.c_uint32, C.c_void_p]
        assert _LIB.lv_field_count() == len(FIELDS)
    return _LIB


def classify(cb, p, ambient, cube, num_dir_lights, pcf_radius, flags, row0=0, rows=None):
    """The per-lane predicates (FIELDS) of every pixel of rows [row0, row0 + rows) of one lighting call over the float4 planes p:
    (H, W, len(FIELDS)) uint8, rows outside the range 0."""
    h, w = p["depth"].shape
    rows = h - row0 if rows is None else rows
    out = np.zeros((h, w, len(FIELDS)), np.uint8)
    g0 = np.ascontiguousarray(p["g0"], np.float32); g2 = np.ascontiguousarray(p["g2"], np.float32)
    d = np.ascontiguousarray(p["depth"], np.uint32); s = np.ascontiguousarray(p["shadow"], np.uint32)
    a = np.ascontiguousarray(ambient, np.uint16); c = np.ascontiguousarray(cube, np.uint8)
    sh = (C.c_void_p * 4)(*[s[k].ctypes.data for k in range(4)])
    load().lv_classify(C.addressof(cb), g0.ctypes.data, g2.ctypes.data, d.ctypes.data, a.ctypes.data, sh, s.shape[1], c.ctypes.data, CUBE_DIM,
                       w, h, row0, rows, num_dir_lights, pcf_radius, int(flags), out.ctypes.data)
    return out


# ---- wavefronts --------------------------------------------------------------------------------------------------------------------
def wave_pixels(w, row0, rows, quads):
    """(waves, 64) flat pixel indices y * w + x of the lanes of every wavefront of a lighting launch over rows [row0, row0 + rows) of a
    frame w pixels wide, -1 for a lane with x >= w or y >= row0 + rows: grid_for's 64 x 4 tiles anchored at row0, and inside a tile
    light_tile_pixel's footprint -- 64 x 1 pixels per wavefront, or 32 x 2 with `quads` (the derivative chain).  Wavefront
    (by * nbx + bx) * 4 + wave; the order in which the device visits the tiles does not matter to a vote."""
    nbx, nby = (w + 63) // 64, (rows + 3) // 4
    by, bx, wave, lane = np.meshgrid(np.arange(nby), np.arange(nbx), np.arange(4), np.arange(64), indexing="ij")
    if quads:
        x = bx * 64 + (wave & 1) * 32 + (lane & 31)
        y = row0 + by * 4 + (wave >> 1) * 2 + (lane >> 5)
    else:
        x = bx * 64 + lane
        y = row0 + by * 4 + wave
    idx = np.where((x < w) & (y < row0 + rows), y * w + x, -1)
    return idx.reshape(-1, 64)


KINDS = ("ALL", "NONE", "ONE_OUT", "ONE_IN", "MIXED", "NO_VOTERS")


def kinds(voters, bits):
    """Per wavefront: the kind of a vote with `voters` (waves, 64) voting and `bits` their answers, and the lane that is alone (the one
    false lane of ONE_OUT, the one true lane of ONE_IN; -1 otherwise).  Two voters that disagree are ONE_OUT."""
    nv = voters.sum(1)
    t = voters & bits
    nt = t.sum(1)
    f = voters & ~bits
    kind = np.full(len(nv), KINDS.index("MIXED"))
    kind[nt == 1] = KINDS.index("ONE_IN")
    kind[nt == nv - 1] = KINDS.index("ONE_OUT")
    kind[nt == 0] = KINDS.index("NONE")
    kind[nt == nv] = KINDS.index("ALL")
    kind[nv == 0] = KINDS.index("NO_VOTERS")
    lane = np.full(len(nv), -1)
    out = kind == KINDS.index("ONE_OUT")
    lane[out] = f[out].argmax(1)
    one = kind == KINDS.index("ONE_IN")
    lane[one] = t[one].argmax(1)
    return kind, lane


VOTES = ("1", "2", "3", "4", "5", "6", "7", "8", "9", "10", "11", "12")


def wave_votes(fields, idx, pcf_radius, flags, chain, shadow_w_is_one=True, gloss=False):
    """Every sub-vote the wavefronts idx (wave_pixels) of a call take, in light_pixel's order: a list of (vote, sub, voters, bits,
    idle) with voters and bits (waves, 64) bool -- bits also holds what a lane that does not vote WOULD answer -- and idle = the
    lanes that are in the frame but on the other side of the coverage test (sky lanes for a vote of lit pixels and the reverse).
    fields: classify() of the call."""
    live = idx >= 0
    flat = fields.reshape(-1, len(FIELDS))

    def f(name):
        return np.where(live, flat[np.maximum(idx, 0), F[name]], 0)

    def b(name):
        return f(name) == 1

    nw = len(idx)
    cov = live & b("COVERED")
    res = []

    def add(vote, sub, voters, bits, idle=None):
        res.append((vote, sub, voters, bits & live, live & ~cov if idle is None else idle))

    def unanimous(voters, bits):
        return voters.any(1) & (bits | ~voters).all(1)

    j = f("J")
    packed = np.zeros(nw, bool)
    if pcf_radius == 0.0 and not (flags & FIX_Q1) and shadow_w_is_one:          # cascade_uniform_test
        first = cov.argmax(1)
        J = j[np.arange(nw), first]                                            # readfirstlane: the first active lane's
        bits10 = (j == J[:, None]) & b("P10")
        add("10", "", cov, bits10)
        packed = unanimous(cov, bits10)
    pk = cov & packed[:, None]
    add("11", "", pk, b("P11"))
    rim = pk & ~unanimous(pk, b("P11"))[:, None]
    add("1", "a", rim, b("P1A"))
    add("1", "b", rim, b("P1B"))
    add("12", "", pk, b("P12"))
    edge = pk & ~unanimous(pk, b("P12"))[:, None]
    p2 = np.stack([b("P2_%d" % k) for k in range(4)], -1)
    own = np.take_along_axis(p2, np.minimum(j, 3)[..., None], -1)[..., 0]
    nxt = np.take_along_axis(p2, np.minimum(j + 1, 3)[..., None], -1)[..., 0]
    add("2", "packed a", edge, own)
    add("2", "packed b", edge, nxt)
    gen = cov & ~packed[:, None] & (j != 4)                                     # cascade_shadow, past its `j == 4` return
    add("8", "", gen, b("P8"))
    needs = f("NEEDS")
    for k in range(4):
        nk = ((needs >> k) & 1) == 1
        add("9", "cascade %d" % k, gen, ~nk)
        if pcf_radius == 0.0:
            add("2", "cascade %d" % k, gen & nk, b("P2_%d" % k))
        else:
            add("3", "cascade %d" % k, gen & nk, b("P3_%d" % k))
    add("6", "", cov, b("P6"))
    add("7", "", cov, b("P7"))
    sky = live & ~cov if flags & SKY else np.zeros_like(cov)
    if chain:
        add("5", "lit", cov, b("P5"))
        add("5", "sky", sky, b("P5"), cov)
        add("4", "lit", cov & unanimous(cov, b("P5"))[:, None], b("P4"))
        add("4", "sky", sky & unanimous(sky, b("P5"))[:, None], b("P4"), cov)
    else:
        if not gloss:                                   # CubeGloss addresses both of its levels with clamps: no vote
            add("4", "lit", cov, b("P4"))
        add("4", "sky", sky, b("P4"), cov)
    return res


# ---- the corpus --------------------------------------------------------------------------------------------------------------------
# Where a frame puts what (all frames alike):
#   rows  0..31  constant per cell of 64 x 2 pixels -- a cell holds the 64 x 1 wavefronts of its two rows and the 32 x 2 wavefronts
#                of its two halves -- drawn from the frame's values, mostly one value per cell, sometimes a handful;
#                rows 16..31: lanes 0..2 of every cell row are sky, so that the first voting lane is lane 3;
#   rows 32..47  one GOOD value per cell and one SPOILER value under one lane of every 64 x 1 wavefront: lane 0, 1 or 31 in the even
#                row, 32, 62 or 63 in the odd row (the same lanes of the 32 x 2 wavefronts of the left and the right half), and lane 7
#                of the partial wavefront (x = 199, in the odd row alone: lane 39 of the 32 x 2 wavefront);
#                rows 44..47: the spoiler lanes are sky, and must not block the shortcut;
#   rows 48..63  per pixel, drawn from the same values, a fifth of them sky.
# GOOD and SPOILER are what the classifier says of a value under the frame's own label, never what its solve intended.
SPOILER_LANES = (0, 1, 31, 32, 62, 63)
EYE = np.array([0.0, 2.0, -15.0])
CASCADE_SPAN = (16.0, 12.0, 20.0, 14.0)             # world units across cascade k's map, centred under the eye
DIST_OF_J = (20.0, 40.0, 65.0, 90.0, 120.0)
DEPTH_SCALE = 2.0 ** -7              # depths of 0.14 .. 0.76: decoded D24 values of both mantissa parities (below 0.5 all are odd)
RIM = (-1.0, -0.5, 0.0, 0.5)
CASCADE_SETS = ((0,), (0, 2), (2, 3), (3, 4), (0, 1, 2, 3, 4))     # the cascades a wavefront of the "cascades" frame holds (votes 9, 10)
EQUAL_DEPTH_DZ = ((18.0, 27.0), (32.0, 47.0), (65.0, 76.0), (82.0, 97.0))      # z - eye.z of pixels that are in cascade k wherever their footprint is


def rim_set(dim):
    return RIM + (dim - 2.5, dim - 2.0, dim - 1.5, dim - 1.0, float(dim))


def constants():
    """The pass constants of the corpus: the default camera's, with four orthographic cascades whose maps look down the z axis --
    u = (x - eye.x) / span_k + 0.5, v likewise in y, depth = (z - eye.z) / 128 -- so that the footprint of a position in cascade J
    and in J + 1 can be set apart."""
    from crychic_renderer_amd import scene
    c = scene.Constants(W, H, shadow_dim=SHADOW_DIM)
    cb = c.pass_cb
    assert np.allclose(list(cb.EyePosW), EYE)
    for k in range(4):
        s = 1.0 / CASCADE_SPAN[k]
        T = [s, 0, 0, 0.5 - EYE[0] * s, 0, s, 0, 0.5 - EYE[1] * s, 0, 0, DEPTH_SCALE, -EYE[2] * DEPTH_SCALE, 0, 0, 0, 1]
        cb.ShadowTransforms[k][:] = [float(np.float32(t)) for t in T]
    return cb


def steps(v):
    """v rounded to binary32, and one step either side."""
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def pos_shadow(k, tx, ty, dist):
    """A position whose texel coordinate in cascade k's map is (tx, ty), at eye distance dist (float64)."""
    dx = ((tx + 0.5) / SHADOW_DIM - 0.5) * CASCADE_SPAN[k]
    dy = ((ty + 0.5) / SHADOW_DIM - 0.5) * CASCADE_SPAN[k]
    dz = np.sqrt(max(dist * dist - dx * dx - dy * dy, 1.0))
    return np.array([EYE[0] + dx, EYE[1] + dy, EYE[2] + dz])


def pos_screen(cb, tx, ty, pz):
    """A position whose texel coordinate in the half-res ambient map is (tx, ty), at world z = pz: ViewProjTex solved for x and y."""
    V = np.array(list(cb.ViewProjTex), np.float64).reshape(4, 4)
    u, v = (tx + 0.5) / (W // 2), (ty + 0.5) / (H // 2)
    sw = V[3, 2] * pz + V[3, 3]                       # the default camera: w depends on z alone
    assert V[3, 0] == 0 and V[3, 1] == 0 and V[0, 1] == 0 and V[1, 0] == 0
    px = (u * sw - V[0, 2] * pz - V[0, 3]) / V[0, 0]
    py = (v * sw - V[1, 2] * pz - V[1, 3]) / V[1, 1]
    return np.array([px, py, pz])


def normal_for(r):
    """The normal that reflects the incident direction (0, 0, 1) -- a pixel straight ahead of the eye -- to r."""
    r = np.asarray(r, np.float64); r = r / np.linalg.norm(r)
    n = r - np.array([0.0, 0.0, 1.0])
    return np.array([1.0, 0.0, 0.0]) if np.linalg.norm(n) < 1e-12 else n / np.linalg.norm(n)


def face_dir(face, sc, tc):
    """The direction whose cube lookup lands on `face` at (sc / ma, tc / ma) (cube_address's table, inverted)."""
    return [(1, -tc, -sc), (-1, -tc, sc), (sc, 1, tc), (sc, -1, -tc), (sc, -tc, 1), (-sc, -tc, -1)][face]


AHEAD = EYE + np.array([0.0, 0.0, 40.0])              # straight ahead of the eye, cascade 1, the middle of every map
VALUE_DT = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3)])


def values(rows):
    v = np.zeros(len(rows), VALUE_DT)
    for k, (p, n) in enumerate(rows):
        v["pos"][k] = p; v["normal"][k] = n
    return v


UP = (0.0, 0.6, -0.8)


def rim_values():
    """Votes 1, 3, 11: the footprint in cascade J, and in J + 1, at the rim of the map on either axis, and at the reach of
    pcf_taps_inside at radii 2.5 / dim and 10 / dim; one binary32 step either side of each."""
    out = [(pos_shadow(J, 30.3, 33.7, DIST_OF_J[J]), UP) for J in range(4)]
    targets = list(rim_set(SHADOW_DIM))
    for radius in (2.5 / SHADOW_DIM, 10.0 / SHADOW_DIM):
        reach = float(np.float32(1.42) * np.float32(radius)) * SHADOW_DIM + 1.0
        targets += [1.0 + reach, SHADOW_DIM - 3.0 - reach]
    for J in range(3):
        for k in (J, J + 1):
            for axis in (0, 1):
                for t in targets:
                    p = pos_shadow(k, t if axis == 0 else 30.3, t if axis == 1 else 33.7, DIST_OF_J[J])
                    for s in steps(p[axis]):
                        q = p.copy(); q[axis] = s
                        out.append((q, UP))
    return values(out)


def content_values(shadow):
    """Votes 2, 12: footprints deep in the lit and in the dark half of the maps, across the edge between them (column 40) with and
    without a fractional weight, and over texels of rows 48.. with the reference depth the texel itself decodes to (and one step either
    side): the pixel is then in the texel's own cascade, `ref <= texel` and d24_threshold's count sit on their boundary."""
    out = []
    for J in range(4):
        for tx in (10.3, 20.0, 30.6, 38.9, 39.0, 39.4, 39.999, 40.0, 40.2, 50.3, 55.0):
            out.append((pos_shadow(J, tx, 20.4, DIST_OF_J[J]), UP))
        for tx, ty in ((19.6, 9.7), (20.0, 10.0), (20.4, 10.3), (19.0, 9.0), (49.5, 29.5), (50.0, 30.0)):      # the one-texel edges
            out.append((pos_shadow(J, tx, ty, DIST_OF_J[J]), UP))
        # (decoded values below 0.5 all have an odd mantissa: the cascades whose depths lie above it get more of them, for both parities)
        more = [(5.0 * i + 0.25 * (i % 4), 49.0 + i) for i in range(1, 12)] if J >= 2 else []
        for tx, ty in [(12.0, 50.0), (12.5, 50.0), (12.0, 50.5), (20.3, 55.6), (30.0, 52.0)] + more:
            k = J
            t = int(shadow[k, int(ty), int(tx)] & 0xFFFFFF)
            ref = t / 16777215.0
            p = pos_shadow(k, tx, ty, DIST_OF_J[J])
            p[2] = EYE[2] + ref / DEPTH_SCALE
            for s in steps(p[2]):
                q = p.copy(); q[2] = s
                out.append((q, UP))
    return values(out)


def cascade_values():
    """Votes 9, 10: eye distances one step either side of 30, 50, 80 and 100, and in the middle of every cascade."""
    out = []
    for d in DIST_OF_J:
        out.append((pos_shadow(0, 30.3, 33.7, d), UP))
    for d in (30.0, 50.0, 80.0, 100.0):
        p = pos_shadow(0, 32.2, 31.1, d)
        for s in steps(p[2]):
            for s2 in steps(s) + [s]:
                q = p.copy(); q[2] = s2
                out.append((q, UP))
    return values(out)


def magnitude_values():
    """Votes 8, 10: position components at 1e15 and 1.2676506e30, one step either side, infinite and NaN."""
    out = [(pos_shadow(J, 30.3, 33.7, DIST_OF_J[J]), UP) for J in range(3)]
    for big in (1.0e15, 1.2676506e30):
        for axis in range(3):
            for sign in (1.0, -1.0):
                for s in steps(big):
                    q = AHEAD.copy(); q[axis] = sign * s
                    out.append((q, UP))
    for bad in (np.inf, -np.inf, np.nan):
        for axis in range(3):
            q = AHEAD.copy(); q[axis] = bad
            out.append((q, UP))
    return values(out)


def first_lane_values():
    """Vote 10 where the lane that supplies J is itself the one that refuses: pixels of cascade 0, and positions with a NaN component
    -- len_from_sq clamps a NaN distance into cascade 0, so such a lane agrees on J and fails `|posW| < 1e15` alone."""
    out = [(pos_shadow(0, tx, ty, d), UP) for tx, ty, d in ((30.3, 33.7, 20.0), (12.6, 40.2, 18.0), (45.1, 22.8, 25.0), (33.0, 31.0, 29.0))]
    for axis in range(3):
        for k in (0, 1):
            q = np.array(out[k][0]); q[axis] = np.nan
            out.append((q, UP))
    q = np.full(3, np.nan)
    out.append((q, UP))
    return values(out)


def ambient_values(cb):
    """Vote 6: the projected footprint at the rim of the 100 x 32 map on either axis, one step either side; vote 7: footprints in
    the part of ambient7() that is all ones, over its single 65534 texels, and in its random part."""
    out = []
    for pz in (5.0, 25.0):
        for tx, ty in ((20.3, 10.6), (40.0, 20.0), (30.5, 5.5), (10.2, 25.9), (50.7, 15.1)):
            out.append((pos_screen(cb, tx, ty, pz), UP))
        for axis, dim in ((0, W // 2), (1, H // 2)):
            for t in rim_set(dim):
                p = pos_screen(cb, t if axis == 0 else 33.3, t if axis == 1 else 12.6, pz)
                for s in steps(p[axis]):
                    q = p.copy(); q[axis] = s
                    out.append((q, UP))
        for tx in (59.2, 59.6, 60.0, 60.4, 61.0, 64.5, 65.0, 70.0, 79.3, 85.5, 93.1):
            for ty in (4.2, 5.0, 9.6, 10.0, 20.7):
                out.append((pos_screen(cb, tx, ty, pz), UP))
    return values(out)


def cube_values():
    """Vote 4: reflections whose footprint lies on a face edge or a corner, on every face, from a pixel straight ahead of the eye."""
    out = [(AHEAD, normal_for(face_dir(f, 0.13, -0.21))) for f in range(6)]
    ts = [t for t in rim_set(CUBE_DIM)] + [CUBE_DIM - 0.5001, -0.4999, 0.999, CUBE_DIM - 1.001]
    for f in range(6):
        for tu in ts:
            for tv in (7.3,) + tuple(ts):
                if tv != 7.3 and (tu not in (-0.5, 0.0, CUBE_DIM - 1.0, float(CUBE_DIM)) or tv not in (-0.5, 0.0, CUBE_DIM - 1.0, float(CUBE_DIM))):
                    continue
                for a, b in ((tu, tv), (tv, tu)):
                    sc, tc = 2.0 * (a + 0.5) / CUBE_DIM - 1.0, 2.0 * (b + 0.5) / CUBE_DIM - 1.0
                    out.append((AHEAD, normal_for(face_dir(f, sc, tc))))
    return values(out)


def cube_pair_values():
    """Vote 4 under the chain, where only a flat wavefront takes it: a reflection half a texel inside a face edge or corner, and
    right after it the one half a texel outside -- less than a texel apart, so the pair stays magnified."""
    out = []
    lo, hi = (0.4, -0.2), (CUBE_DIM - 1.4, CUBE_DIM - 0.8)
    for f in range(6):
        for a, b in ((lo, (7.3, 7.3)), (hi, (7.3, 7.3)), ((7.3, 7.3), lo), ((7.3, 7.3), hi), (lo, lo), (hi, hi), (lo, hi), (hi, lo)):
            for k in (0, 1):
                sc, tc = 2.0 * (a[k] + 0.5) / CUBE_DIM - 1.0, 2.0 * (b[k] + 0.5) / CUBE_DIM - 1.0
                out.append((AHEAD, normal_for(face_dir(f, sc, tc))))
    return values(out)


def flat_values():
    """Vote 5: a flat wavefront of reflections along (0, 0, 1), and neighbours tilted by d in x: 8 d is the footprint in texels of a
    16-texel face, so around d = 1 / 8 the flat lane still sees a magnified lookup while the tilted lane (whose major axis is a
    little shorter) does not -- exactly one lane of the wavefront leaves level 0.  Which d does that is the classifier's to say."""
    out = [(AHEAD, normal_for((0.0, 0.0, 1.0)))]
    for d in np.linspace(0.1215, 0.1265, 41):
        out.append((AHEAD, normal_for((d, 0.0, np.sqrt(1.0 - d * d)))))
    for d in (0.01, 0.05, 0.3, 0.6):
        out.append((AHEAD, normal_for((d, -d, np.sqrt(1.0 - 2 * d * d)))))
    return values(out)


def shadow_maps(kind, rng):
    """random: every texel random (half of each map mostly lit, as fuzz_util's).  content: columns below 40 all 0xFFFFFF, the others all
    0, with one isolated texel of the other kind in either half ((20, 10) dark, (50, 30) lit); rows 48.. of cascade k: decoded values that are reference depths of pixels in cascade k (EQUAL_DEPTH_DZ)."""
    if kind == "random":
        s = rng.integers(0, 1 << 24, size=(4, SHADOW_DIM, SHADOW_DIM), dtype=np.uint32)
        s[:, : SHADOW_DIM // 2] |= 0x00F00000
    else:
        s = np.zeros((4, SHADOW_DIM, SHADOW_DIM), np.uint32)
        s[:, :, :40] = 0xFFFFFF
        s[:, 10, 20] = 0                    # one dark texel in the lit half, one lit texel in the dark half
        s[:, 30, 50] = 0xFFFFFF
        for k, (lo, hi) in enumerate(EQUAL_DEPTH_DZ):
            s[k, 48:] = rng.integers(int(lo * DEPTH_SCALE * 16777215), int(hi * DEPTH_SCALE * 16777215), size=(SHADOW_DIM - 48, SHADOW_DIM), dtype=np.uint32)
    return s | (rng.integers(0, 256, size=s.shape, dtype=np.uint32) << 24)        # the stencil byte is ignored


def ambient7(rng):
    """All 65535, with single texels of 65534 in columns 60..79 (every fifth column and row) and random columns 80..99."""
    a = np.full((H // 2, W // 2), 65535, np.uint16)
    a[::5, 60:80:5] = 65534
    a[:, 80:] = rng.integers(0, 65536, size=(H // 2, W // 2 - 80), dtype=np.uint16)
    return a


class Frame:
    """One frame of the corpus: planes (g0, g1, g2, depth, shadow), the ambient map, and which vote it was laid out for."""


def lay_out(name, vals, good, rng, shadow, ambient, pair_of=None, spoil=None, key=None, cells=None):
    """The frame that holds `vals` in the layout above; good: the classifier's answer for each value under the frame's label; spoil:
    the values that serve as spoilers (default: all that are not good).  pair_of: for the spoilers, the good value that has to
    surround each -- one index, or one per value (votes 4 and 5 of the chain: the reflection the spoiler's is measured against).
    key: one number per value; a spoiler is surrounded by a good value of its own key where there is one (the votes of the packed
    cascade path are taken only by wavefronts of one cascade: key = the value's cascade).  cells(pick, sky): rewrites the choice of
    values and the coverage in place before the planes are made (the cascade sets)."""
    gi, si = np.nonzero(good)[0], np.nonzero(~good if spoil is None else spoil)[0]
    assert len(gi) and len(si), (name, len(gi), len(si))
    pick = np.zeros((H, W), np.int64)
    sky = np.zeros((H, W), bool)
    nb = (W + 63) // 64
    for pair in range(16):                                      # rows 0..31
        for b in range(nb):
            r = rng.random()
            if r < 0.45:
                pool = gi[[rng.integers(len(gi))]]
            elif r < 0.75:
                pool = si[[rng.integers(len(si))]]
            else:
                pool = rng.integers(0, len(vals), int(rng.integers(2, 6)))
            pick[2 * pair:2 * pair + 2, 64 * b:64 * b + 64] = rng.choice(pool, size=pick[2 * pair:2 * pair + 2, 64 * b:64 * b + 64].shape)
            if pair >= 8:
                sky[2 * pair:2 * pair + 2, 64 * b:64 * b + 3] = True
    n = 0
    for pair in range(8):                                       # rows 32..47
        y = 32 + 2 * pair
        for b in range(nb):
            if b < nb - 1:
                spots = [(y, 64 * b + SPOILER_LANES[pair % 3]), (y + 1, 64 * b + SPOILER_LANES[3 + pair % 3])]
            else:
                spots = [(y + 1, W - 1)]
            s = si[n % len(si)]; n += 1
            pool = gi if key is None or not (key[gi] == key[s]).any() else gi[key[gi] == key[s]]
            g = pool[rng.integers(len(pool))] if pair_of is None else (pair_of if np.isscalar(pair_of) else pair_of[s])
            pick[y:y + 2, 64 * b:64 * b + 64] = g
            for yy, xx in spots:
                pick[yy, xx] = s
                sky[yy, xx] = pair >= 6
    pick[48:] = rng.integers(0, len(vals), size=(H - 48, W))    # rows 48..63
    sky[48:] = rng.random((H - 48, W)) < 0.2
    if cells is not None:
        cells(pick, sky)
    fr = Frame()
    fr.name = name
    g0 = np.zeros((H, W, 4), np.float32); g2 = np.zeros((H, W, 4), np.float32)
    g0[..., :3] = vals["pos"][pick]; g0[..., 3] = rng.random((H, W))
    g2[..., :3] = vals["normal"][pick]; g2[..., 3] = 1.0
    g1 = rng.random((H, W, 4)).astype(np.float32); g1[..., 3] = 0.1 + 0.8 * g1[..., 3]
    depth = rng.integers(0, 0xFFFFFF, size=(H, W), dtype=np.uint32)
    depth[sky] = 0xFFFFFF
    depth |= rng.integers(0, 256, size=(H, W), dtype=np.uint32) << 24
    fr.planes = {"g0": g0, "g1": g1, "g2": g2, "depth": depth, "shadow": shadow}
    fr.ambient = ambient
    fr.pick, fr.good = pick, good
    return fr


class Config:
    """family "frame": crychic_deferred_light against the oracle; "point shadows": crychic_deferred_light_point_shadows with
    local_lights() against the family's checker (tests/point_shadow_ref) -- its kernels compile the FIX switches in and cull the
    local lights per tile in LDS, the votes of light_pixel are the literal frame's; "general": crychic_deferred_light with the gloss
    lookup, SH ambient and the split-sum table over G1 and G2 as half4 (general_call()) against tests/env_brdf_ref's checker -- no vote
    in its reflection lookup, so vote 4 is taken by sky lanes alone, whose direction is their pixel's (nothing to lay out)."""
    def __init__(self, name, radius, flags, chain=False, family="frame"):
        self.name, self.radius, self.flags, self.chain, self.family = name, radius, flags, chain, family
        self.gloss = bool(flags & GLOSS)


CONFIGS = (Config("frame r=0", 0.0, SKY), Config("frame r=2.5/dim", 2.5 / SHADOW_DIM, SKY), Config("fix Q1 r=0", 0.0, SKY | FIX_Q1),
           Config("chain r=0", 0.0, SKY | (CUBE_LEVELS << 16), chain=True), Config("point shadows", 0.0, SKY, family="point shadows"),
           Config("general, half G1 G2", 0.0, SKY | GLOSS | AMBIENT_SH | ENV_BRDF | (CUBE_LEVELS << 16), family="general"))
N_POINTS, N_SPOTS, N_SHADOWED, LOCAL_DIM = 40, 8, 2, 32
_LOCAL = None


def local_lights():
    """The local lights of the point-shadow configuration: 40 point lights (the first 2 with cube shadows) and 8 spot lights (the
    first 2 with shadow maps) among the positions of the corpus, random D24 faces and maps of 32 texels, the product's own
    transform builders; cb / pcb: the corpus's constants with the spot transforms in slots 4 and 5.  A dict, built once."""
    global _LOCAL
    if _LOCAL is not None:
        return _LOCAL
    import fuzz_util
    from local_lights_util import random_maps, spot_transforms, transposed, with_transforms
    from point_shadow_lib import point_transforms, random_cubes
    rng = np.random.default_rng(77)

    def lights(n):
        rec = np.zeros(n, fuzz_util.LIGHT_DT)
        rec["Position"] = np.stack([EYE[0] + rng.uniform(-8, 8, n), EYE[1] + rng.uniform(-6, 6, n), EYE[2] + rng.uniform(15, 110, n)], 1)
        rec["FalloffEnd"] = rng.choice(np.array([10.0, 30.0], np.float32), n)
        rec["FalloffStart"] = 1.0
        rec["Strength"] = rng.choice(np.array([0.1, 1.0, 2.4], np.float32), (n, 3))
        d = rng.standard_normal((n, 3)); rec["Direction"] = d / np.linalg.norm(d, axis=1, keepdims=True)
        rec["SpotPower"] = rng.choice(np.array([0.0, 1.0, 8.0], np.float32), n)
        return fuzz_util.lights_from_records(rec)
    points, spots = lights(N_POINTS), lights(N_SPOTS)
    cb, pcb = with_transforms(corpus().cb, [transposed(st) for _, _, st in spot_transforms(spots, N_SHADOWED)])
    _LOCAL = dict(points=points, spots=spots, maps=random_maps(N_SHADOWED, LOCAL_DIM, 5), cubes=random_cubes(N_SHADOWED, LOCAL_DIM, 6),
                  projs=[sp.reshape(-1) for _, _, sp in point_transforms(points, N_SHADOWED, LOCAL_DIM)], cb=cb, pcb=pcb)
    return _LOCAL


_GENERAL = None


def general_call():
    """What the general-family configuration adds to the corpus: the cube map's chain followed by an environment tail with random SH
    coefficients and a random split-sum table (tests/env_brdf_lib.with_table).  Built once."""
    global _GENERAL
    if _GENERAL is None:
        import env_brdf_lib
        rng = np.random.default_rng(91)
        table = rng.integers(0, 2 ** 32, 1024, dtype=np.uint64).astype(np.uint32)
        coeffs = rng.uniform(-0.5, 1.0, (9, 4)).astype(np.float32)
        _GENERAL = env_brdf_lib.with_table(corpus().chain, CUBE_DIM, CUBE_LEVELS, table, coeffs)
    return _GENERAL


def planes_of(fr, cfg):
    """The frame's planes as cfg's call stores them (general: G1 and G2 as half4), and as float32 (what a checker reads)."""
    import gbuffer_f16_lib as gf
    if cfg.family != "general":
        return fr.planes, fr.planes
    packed = gf.pack_planes(fr.planes, HALF_G1_G2)
    return packed, gf.widen_planes(packed)


def light_kwargs():
    lo = local_lights()
    return {k: lo[k] for k in ("points", "spots", "maps", "cubes", "projs")}
NUM_DIR_LIGHTS = 3


class Corpus:
    pass


_CORPUS = None


def corpus():
    """The frames, the constants and the cube map (and its 5-level chain) every configuration runs over.  Built once."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    from crychic_renderer_amd import geometry
    rng = np.random.default_rng(20240613)
    co = Corpus()
    co.cb = constants()
    co.cube = rng.integers(0, 256, (6, CUBE_DIM, CUBE_DIM, 4), dtype=np.uint8)
    co.chain, levels = geometry.cube_mip_chain(co.cube)
    assert levels == CUBE_LEVELS
    s_random, s_content = shadow_maps("random", rng), shadow_maps("content", rng)
    a_random = rng.integers(0, 65536, size=(H // 2, W // 2), dtype=np.uint16)
    a_ones = ambient7(rng)

    def label(vals, shadow, ambient, cfg, fn):
        """fn(fields of each value) under configuration cfg: the values tiled over a frame of the corpus's own size, all covered."""
        assert len(vals) <= W * H
        pick = np.arange(W * H) % len(vals)
        g0 = np.zeros((H, W, 4), np.float32); g2 = np.zeros((H, W, 4), np.float32)
        g0[..., :3] = vals["pos"][pick].reshape(H, W, 3); g2[..., :3] = vals["normal"][pick].reshape(H, W, 3)
        p = {"g0": g0, "g2": g2, "depth": np.zeros((H, W), np.uint32), "shadow": shadow}
        fl = classify(co.cb, p, ambient, co.cube, NUM_DIR_LIGHTS, cfg.radius, cfg.flags).reshape(-1, len(FIELDS))[:len(vals)].astype(np.int64)
        return fn(fl)

    def needed(fl, name):
        ok = np.ones(len(fl), bool)
        for k in range(4):
            ok &= (((fl[:, F["NEEDS"]] >> k) & 1) == 0) | (fl[:, F["%s_%d" % (name, k)]] == 1)
        return ok

    r0, rr, q1 = CONFIGS[0], CONFIGS[1], CONFIGS[2]
    frames = []
    v = rim_values()
    jv = label(v, s_random, a_random, r0, lambda fl: fl[:, F["J"]])
    frames.append(lay_out("rim, vote 11", v, label(v, s_random, a_random, r0, lambda fl: fl[:, F["P11"]] == 1), rng, s_random, a_random, key=jv))
    # vote 1 is taken only where vote 11 is refused: cells whose footprint leaves the map of cascade J + 1 alone, spoilers that leave J's
    frames.append(lay_out("rim, vote 1", v, label(v, s_random, a_random, r0, lambda fl: (fl[:, F["P10"]] == 1) & (fl[:, F["P1A"]] == 1) & (fl[:, F["P1B"]] == 0)),
                          rng, s_random, a_random, spoil=label(v, s_random, a_random, r0, lambda fl: (fl[:, F["P10"]] == 1) & (fl[:, F["P1A"]] == 0)), key=jv))
    frames.append(lay_out("rim, vote 3", v, label(v, s_random, a_random, rr, lambda fl: needed(fl, "P3")), rng, s_random, a_random))
    v = content_values(s_content)
    jv = label(v, s_content, a_random, r0, lambda fl: fl[:, F["J"]])
    frames.append(lay_out("content, vote 12", v, label(v, s_content, a_random, r0, lambda fl: fl[:, F["P12"]] == 1), rng, s_content, a_random, key=jv))
    frames.append(lay_out("content, vote 2", v, label(v, s_content, a_random, q1, lambda fl: needed(fl, "P2")), rng, s_content, a_random, key=jv))
    v = cascade_values()
    jv = label(v, s_random, a_random, r0, lambda fl: fl[:, F["J"]])

    def cascade_cells(pick, sky):
        """Rows 0..31: the cells cycle through CASCADE_SETS -- every pixel drawn from the values of the set's cascades, each cascade at
        both ends of both rows so that no wavefront of the cell misses one -- and through FIRST_IN_3: cascade 0 with lane 0 of the even
        row in cascade 3."""
        r = np.random.default_rng(5150)
        of = [np.nonzero(jv == j)[0] for j in range(5)]
        n = 0
        for pair in range(16):
            for b in range((W + 63) // 64):
                ys, xs = slice(2 * pair, 2 * pair + 2), slice(64 * b, min(64 * b + 64, W))
                kind = n % (len(CASCADE_SETS) + 1); n += 1
                members = (0,) if kind == len(CASCADE_SETS) else CASCADE_SETS[kind]
                shape = pick[ys, xs].shape
                js = r.choice(members, size=shape)
                for i, j in enumerate(members):             # every member in the first lanes of both halves of both rows
                    js[:, 3 + i::32] = j                    # (behind the sky lanes of rows 16..31)
                pick[ys, xs] = np.vectorize(lambda j: r.choice(of[j]))(js)
                if kind == len(CASCADE_SETS):
                    pick[2 * pair, 64 * b] = r.choice(of[3])
                    sky[2 * pair, 64 * b] = False
    frames.append(lay_out("cascades", v, jv == 0, rng, s_random, a_random, cells=cascade_cells))
    v = magnitude_values()
    frames.append(lay_out("magnitudes", v, label(v, s_random, a_random, r0, lambda fl: (fl[:, F["P10"]] == 1) & (fl[:, F["J"]] == 1)), rng, s_random, a_random))
    frames.append(lay_out("magnitudes, vote 8", v, label(v, s_random, a_random, r0, lambda fl: (fl[:, F["P8"]] == 1) & (fl[:, F["J"]] < 4)), rng, s_random,
                          a_random, spoil=label(v, s_random, a_random, r0, lambda fl: (fl[:, F["P8"]] == 0) & (fl[:, F["J"]] < 4))))
    v = ambient_values(co.cb)
    frames.append(lay_out("ambient, vote 6", v, label(v, s_random, a_random, r0, lambda fl: fl[:, F["P6"]] == 1), rng, s_random, a_random))
    frames.append(lay_out("ambient, vote 7", v, label(v, s_random, a_ones, r0, lambda fl: fl[:, F["P7"]] == 1), rng, s_random, a_ones))
    v = cube_values()
    frames.append(lay_out("cube, vote 4", v, label(v, s_random, a_random, r0, lambda fl: fl[:, F["P4"]] == 1), rng, s_random, a_random))
    v = cube_pair_values()
    inside = label(v, s_random, a_random, r0, lambda fl: fl[:, F["P4"]] == 1)
    frames.append(lay_out("cube pairs, vote 4 of the chain", v, inside, rng, s_random, a_random, pair_of=np.arange(len(v)) - 1,
                          spoil=~inside & np.roll(inside, 1) & (np.arange(len(v)) % 2 == 1)))
    # vote 5: a tilted lane among flat ones leaves level 0 alone when the flat lanes still see a magnified lookup: ask the classifier
    # about every tilt d, as the one covered x neighbour of the flat value
    v = flat_values()
    g0 = np.zeros((H, W, 4), np.float32); g2 = np.zeros((H, W, 4), np.float32)
    g0[..., :3] = v["pos"][0]; g2[..., :3] = v["normal"][0]
    spots = [(2 * (k // 90), 2 * (k % 90) + 1) for k in range(1, len(v))]
    for k, (y, x) in enumerate(spots):
        g2[y, x, :3] = v["normal"][k + 1]
    fl = classify(co.cb, {"g0": g0, "g2": g2, "depth": np.zeros((H, W), np.uint32), "shadow": s_random}, a_random, co.chain, NUM_DIR_LIGHTS, 0.0,
                  CONFIGS[3].flags)
    alone = np.array([True] + [not (fl[y, x, F["P5"]] == 0 and fl[y, x - 1, F["P5"]] == 1 and fl[y + 1, x, F["P5"]] == 1) for y, x in spots])
    frames.append(lay_out("flat quads, vote 5", v, alone, rng, s_random, a_random, pair_of=0))
    v = first_lane_values()
    frames.append(lay_out("first lane, vote 10", v, label(v, s_random, a_random, r0, lambda fl: (fl[:, F["P10"]] == 1) & (fl[:, F["J"]] == 0)), rng, s_random, a_random,
                          spoil=label(v, s_random, a_random, r0, lambda fl: (fl[:, F["P10"]] == 0) & (fl[:, F["J"]] == 0))))
    co.frames = frames
    _CORPUS = co
    return co


def cube_of(co, cfg):
    return general_call() if cfg.family == "general" else (co.chain if cfg.chain else co.cube)


def call_fields(co, fr, cfg, row0=0, rows=None):
    return classify(co.cb, planes_of(fr, cfg)[1], fr.ambient, cube_of(co, cfg), NUM_DIR_LIGHTS, cfg.radius, cfg.flags, row0, rows)


# ---- the census --------------------------------------------------------------------------------------------------------------------
def census(co=None):
    """Per (configuration, vote): what the wavefronts of the whole corpus are, every sub-vote pooled.  A dict
    [(config name, vote)] -> {"kinds": counts by KINDS, "one_out": counts by lane of the ONE_OUT wavefronts (full wavefronts),
    "one_out_partial": the same for the wavefronts of 8 (2 x 8) live lanes, "all_partial": ALL wavefronts among those,
    "all_uncovered_spoiler": ALL wavefronts with a lane that is in the frame, does not vote and would have answered no,
    "all_first_not_0": ALL wavefronts whose first voting lane is not lane 0}.  Row ranges regroup nothing -- their tiles are anchored
    at row0 and every range of ROW_RANGES starts on an even row -- so the whole frame's wavefronts are every call's."""
    co = co or corpus()
    out = {}
    for cfg in CONFIGS:
        idx = wave_pixels(W, 0, H, cfg.chain)
        partial = (idx >= 0).sum(1) < 64
        for v in VOTES:
            out[(cfg.name, v)] = {"kinds": np.zeros(len(KINDS), np.int64), "one_out": {}, "one_out_partial": {}, "all_partial": 0,
                                  "all_uncovered_spoiler": 0, "all_first_not_0": 0}
        for fr in co.frames:
            fields = call_fields(co, fr, cfg)
            for vote, sub, voters, bits, would in wave_votes(fields, idx, cfg.radius, cfg.flags, cfg.chain, gloss=cfg.gloss):
                c = out[(cfg.name, vote)]
                kind, lane = kinds(voters, bits)
                c["kinds"] += np.bincount(kind, minlength=len(KINDS))
                is_all = kind == KINDS.index("ALL")
                for part, key in ((False, "one_out"), (True, "one_out_partial")):
                    for l in lane[(kind == KINDS.index("ONE_OUT")) & (partial == part)]:
                        c[key][int(l)] = c[key].get(int(l), 0) + 1
                c["all_partial"] += int((is_all & partial).sum())
                c["all_uncovered_spoiler"] += int((is_all & (would & ~bits).any(1)).sum())
                c["all_first_not_0"] += int((is_all & (voters.argmax(1) != 0)).sum())
    return out


def reachable(cfg, vote):
    """Can a wavefront of configuration cfg take `vote` at all?  The packed cascade path (10, 11, 12, and 1 on its rim) exists only
    at the literal radius 0 without CRYCHIC_FIX_Q1; the general taps (3) only at a radius that is not 0; the flat vote (5) only for
    the derivative chain."""
    packed = cfg.radius == 0.0 and not (cfg.flags & FIX_Q1)
    return {"1": packed, "10": packed, "11": packed, "12": packed, "3": cfg.radius != 0.0, "2": cfg.radius == 0.0, "5": cfg.chain}.get(vote, True)


def laid_out(cfg, vote):
    """Does the corpus drive `vote` under cfg?  Not vote 4 of the general family: only sky lanes take it there."""
    return reachable(cfg, vote) and not (cfg.family == "general" and vote == "4")


def census_text(cen):
    lines = ["wave votes of the lighting kernels over the corpus of tests/light_votes_lib.py (%d x %d, every frame, whole-frame calls)" % (W, H),
             "per (configuration, vote): wavefronts by kind, sub-votes pooled; ONE_OUT by the lane that refuses (full wavefronts | the",
             "partial wavefront); ALL wavefronts that are partial / hold an uncovered lane with the spoiler value / start at a lane other than 0", ""]
    for (cfg, vote), c in cen.items():
        k = c["kinds"]
        lines.append("%-16s vote %-3s %s" % (cfg, vote, "  ".join("%s %d" % (n, k[i]) for i, n in enumerate(KINDS))))
        if k[:5].sum():
            lines.append("%-16s          one out at %s | %s; ALL: partial %d, uncovered spoiler %d, first voter not lane 0 %d" % (
                "", " ".join("%d:%d" % kv for kv in sorted(c["one_out"].items())) or "-",
                " ".join("%d:%d" % kv for kv in sorted(c["one_out_partial"].items())) or "-", c["all_partial"], c["all_uncovered_spoiler"], c["all_first_not_0"]))
    return "\n".join(lines) + "\n"


def chain_config():
    return [c for c in CONFIGS if c.chain][0]


def quad_census(co=None):
    """Vote 13 (light_tiles.hpp:70) under the chain configuration.  "covered": the 2 x 2 quads of the corpus by their number of covered
    pixels, 0..4; "minified": those of them in which a covered pixel has lod != 0 -- with one covered pixel there is no covered
    neighbour and no derivative, so that entry must be 0.  (No quad is split by the end of a call: the API takes even frame heights
    only, and of the chain an even row0 and even rows.)"""
    co = co or corpus()
    cfg = chain_config()
    out = {k: np.zeros(5, np.int64) for k in ("covered", "minified")}

    def count(cov, lod, a, b):
        q = lambda m: m[0::2, 0::2].astype(int) + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2]
        nq = q(cov)
        out[a] += np.bincount(nq.reshape(-1), minlength=5)
        out[b] += np.bincount(nq[q(cov & lod) > 0].reshape(-1), minlength=5)
    for fr in co.frames:
        fl = call_fields(co, fr, cfg)
        count(fl[..., F["COVERED"]] == 1, fl[..., F["P5"]] == 0, "covered", "minified")
    return out


def cascade_set_census(co=None):
    """Votes 9, 10: per footprint (64 x 1, 32 x 2), how many wavefronts of the corpus hold exactly the cascades of each of CASCADE_SETS
    among their covered lanes, and ("first in 3") how many have their first voting lane in cascade 3 and every other one in 0."""
    co = co or corpus()
    out = {}
    for quads in (False, True):
        idx = wave_pixels(W, 0, H, quads)
        live = idx >= 0
        n = {s: 0 for s in CASCADE_SETS}; n["first in 3"] = 0
        for fr in co.frames:
            fl = call_fields(co, fr, CONFIGS[0]).reshape(-1, len(FIELDS))
            cov = live & (fl[np.maximum(idx, 0), F["COVERED"]] == 1)
            j = fl[np.maximum(idx, 0), F["J"]]
            has = np.stack([(cov & (j == k)).any(1) for k in range(5)], 1)
            for s in CASCADE_SETS:
                n[s] += int((has == np.array([k in s for k in range(5)])).all(1).sum())
            first = cov.argmax(1)
            rest = cov.copy(); rest[np.arange(len(idx)), first] = False
            n["first in 3"] += int((cov.any(1) & (j[np.arange(len(idx)), first] == 3) & (rest.sum(1) >= 7) & ((j == 0) | ~rest).all(1)).sum())
        out["32 x 2" if quads else "64 x 1"] = n
    return out


def census_report(co=None):
    """The text of profiles/light_votes_census.txt."""
    q = quad_census(co)
    text = census_text(census(co))
    text += "\nvote 13, chain: 2 x 2 quads by covered pixels 0..4: %s; of them with lod != 0 on a covered pixel: %s\n" % (
        " ".join(map(str, q["covered"])), " ".join(map(str, q["minified"])))
    for fp, n in cascade_set_census(co).items():
        text += "votes 9, 10, %s wavefronts that hold exactly the cascades %s\n" % (fp, ", ".join("%s: %d" % (k if isinstance(k, str) else set(k), v) for k, v in n.items()))
    return text


def equal_depth_values(hostsim, co=None):
    """How many values of the content frames have a reference depth that IS the decoded value (devmath d24_to_float) of the top-left
    texel of their footprint in a cascade they need: the boundary of gsamShadow's `ref <= texel` and of d24_threshold.  [even, odd]
    by the lowest mantissa bit of that depth (a one-bit error in the reference moves an even one up across the texel, an odd one down)."""
    co = co or corpus()
    shadow = co.frames[[fr.name for fr in co.frames].index("content, vote 2")].planes["shadow"]
    n = [0, 0]
    for q in content_values(shadow)["pos"]:
        d = np.float32(np.float32(q[2]) * np.float32(DEPTH_SCALE)) + np.float32(-EYE[2] * DEPTH_SCALE)
        dist = np.linalg.norm(q.astype(np.float64) - EYE)
        j = sum(dist >= r for r in (30.0, 50.0, 80.0, 100.0))
        for k in (j, j + 1):
            if k < 4:
                tx, ty = (((q[c] - EYE[c]) / CASCADE_SPAN[k] + 0.5) * SHADOW_DIM - 0.5 for c in (0, 1))
                if 0 <= tx < SHADOW_DIM - 1 and 0 <= ty < SHADOW_DIM - 1:
                    if hostsim.lib.hs_d24_to_float(int(shadow[k, int(np.floor(ty)), int(np.floor(tx))] & 0xFFFFFF)) == d:
                        n[int(d.view(np.uint32)) & 1] += 1
    return n


# ---- references --------------------------------------------------------------------------------------------------------------------
_REFS = {}


def reference(oracle, k, cfg, row0, rows):
    """The oracle's (or the family checker's) RGBA8 and radiance of frame k under cfg over rows [row0, row0 + rows); computed once,
    never written to."""
    import oracle_lib
    key = (k, cfg.name, row0, rows)
    if key not in _REFS:
        co = corpus()
        fr = co.frames[k]
        p, amb = fr.planes, fr.ambient
        if cfg.family == "general":
            import env_brdf_lib
            ref, rad = env_brdf_lib.load().checker_light(oracle_lib.as_oracle_cb(co.cb, oracle_lib.OrPassConstants), dict(planes_of(fr, cfg)[1], cube=cube_of(co, cfg)),
                                                         fr.ambient, NUM_DIR_LIGHTS, cfg.radius, cfg.flags, row0=row0, rows=rows, cube_dim=CUBE_DIM)
            ref.setflags(write=False); rad.setflags(write=False)
            _REFS[key] = (ref, rad)
            return _REFS[key]
        if cfg.family == "point shadows":
            import point_shadow_lib
            ref, rad = point_shadow_lib.load().checker(local_lights()["pcb"], dict(p, cube=cube_of(co, cfg)), fr.ambient, NUM_DIR_LIGHTS, cfg.radius,
                                                       cfg.flags, row0=row0, rows=rows, cube_dim=CUBE_DIM, **light_kwargs())
            ref.setflags(write=False); rad.setflags(write=False)
            _REFS[key] = (ref, rad)
            return _REFS[key]
        ocb = oracle_lib.as_oracle_cb(co.cb, oracle_lib.OrPassConstants)
        ref, rad = oracle.deferred_light(ocb, p["g0"], p["g1"], p["g2"], p["depth"], amb, p["shadow"], cube_of(co, cfg), NUM_DIR_LIGHTS,
                                         cfg.radius, sky=True, want_radiance=True, row0=row0, rows=rows, fixes=cfg.flags & 0x700,
                                         cube_dim=CUBE_DIM, cube_levels=CUBE_LEVELS if cfg.chain else 0)
        ref.setflags(write=False); rad.setflags(write=False)
        _REFS[key] = (ref, rad)
    return _REFS[key]


if __name__ == "__main__":      # python tests/light_votes_lib.py: writes profiles/light_votes_census.txt
    import sys
    sys.path.insert(0, ROOT)
    with open(CENSUS_FILE, "w") as fh:
        fh.write(census_report())
