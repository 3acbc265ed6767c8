"""Float64 / int64 restatements in numpy of the four depth-reading post passes -- volumetric fog, depth of field, temporal
anti-aliasing, motion blur -- written from the text of include/crychic_hip.h alone (TEST INFRASTRUCTURE ONLY).  Nothing here calls a
checker, a kernel body or a host build: of taa_lib, motion_blur_lib, fog_lib and dof_lib only the Case / Frame containers and the
parameter dictionaries are used, as data.

The binary32 inputs (matrices, parameters, and the host constants the header defines as binary32 values) are taken at their binary32
value and promoted; every other operation is float64, with an IEEE division wherever the header says rcp.  The integer back ends are
exact.  Every restated function takes `mutation`: the name of one deliberate misreading (MUTATIONS), for test_restatement_bites."""
import math

import numpy as np

BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64)
F32_MIN_NORMAL, F32_MAX = 2.0 ** -126, float(np.finfo(np.float32).max)

# One deliberate misreading of the header each, selected by `mutation=`:
#   front        no_half_pixel: (float)px without + 0.5;  ny_sign: ny = fma(py + 0.5, +sy, 1);  d24_pow2: d = v / 16777216;
#                ivp_untransposed: InvViewProj read as if it were not stored transposed
#   motion_blur  hw_w_minus_1: hw = 0.5 (W - 1);  shutter_255: sh = shutter / 255;  euclid_clamp: m = sqrt(s_x^2 + s_y^2);
#                cur_prev_swapped;  tile_first_lane: a tile's tie of lengths goes to the first lane, not the largest word;
#                dist_strict: 2 dist < lenY;  bayer_transposed: B[px & 3][py & 3]
#   taa          xmax_256w: xmax = 256 W;  b3_ge: b[3] >= 0;  lohi_row_range: the 3 x 3 clamped to the call's rows;
#                round_32767: hv with + 32767;  blend_swapped: hc blend + c 256 (256 - blend)
#   dof          ds_ge_dp: D_s >= D_p;  k_plus_7: k = c_e + 7 - d16;  inv_max_15: inv from max(c, 15)^2;
#                frame_is_row_range: a sample outside the call's rows is skipped
#   fog          cascade_le: j from t <= 30, 50, 80, 100;  jit_no_half: jit = B / 16;  sz_lt_map: lit iff s.z < map;
#                t_round_32767: T with + 32767;  lc_unclamped: Lc = L
MUTATIONS = {
    "front": ("no_half_pixel", "ny_sign", "d24_pow2", "ivp_untransposed"),
    "motion_blur": ("hw_w_minus_1", "shutter_255", "euclid_clamp", "cur_prev_swapped", "tile_first_lane", "dist_strict", "bayer_transposed"),
    "taa": ("xmax_256w", "b3_ge", "lohi_row_range", "round_32767", "blend_swapped"),
    "dof": ("ds_ge_dp", "k_plus_7", "inv_max_15", "frame_is_row_range"),
    "fog": ("cascade_le", "jit_no_half", "sz_lt_map", "t_round_32767", "lc_unclamped"),
}


def f32(x):
    """The binary32 value of x, promoted."""
    return float(np.float32(x))


def _columns(m, mutation=None):
    """Row c = the four floats of column c of the row-vector matrix (the header's `m + 4c`), as float64."""
    M = np.asarray(m, np.float32).astype(np.float64).reshape(4, 4)
    return M.T.copy() if mutation == "ivp_untransposed" else M


def _abnormal(*arrays):
    """Where any finite, non-zero value lies outside binary32's normal range."""
    bad = np.zeros(np.shape(arrays[0]), bool)
    for a in arrays:
        m = np.abs(a)
        bad |= np.isfinite(a) & (a != 0) & ((m < F32_MIN_NORMAL) | (m > F32_MAX))
    return bad


# ---- the shared front end ------------------------------------------------------------------------------------------------------------

def world_point64(ivp, depth, W, H, mutation=None, parts=False):
    """Steps 1 - 3 of crychic_fog: the (H, W, 3) world points of a (H, W) D24 plane through InvViewProj.  parts: (P, h) with the
    (H, W, 4) homogeneous h."""
    with np.errstate(all="ignore"):
        d = (np.asarray(depth).astype(np.int64) & 0xFFFFFF).astype(np.float64) / (16777216.0 if mutation == "d24_pow2" else 16777215.0)
        sx, sy = f32(np.float32(2.0) / np.float32(W)), f32(np.float32(2.0) / np.float32(H))
        half = 0.0 if mutation == "no_half_pixel" else 0.5
        nx = (np.arange(W, dtype=np.float64)[None, :] + half) * sx - 1.0
        ny = (np.arange(H, dtype=np.float64)[:, None] + half) * (sy if mutation == "ny_sign" else -sy) + 1.0
        M = _columns(ivp, mutation)
        h = np.stack([nx * M[c, 0] + ny * M[c, 1] + d * M[c, 2] + M[c, 3] for c in range(4)], axis=-1)
        P = h[..., :3] * (1.0 / h[..., 3])[..., None]
    return (P, h) if parts else P


def project64(P, vp):
    """mulcol1(P, vp + 4c) for c = 0, 1, 3: (x, y, w), each (H, W)."""
    M = _columns(vp)
    return [P[..., 0] * M[c, 0] + P[..., 1] * M[c, 1] + P[..., 2] * M[c, 2] + M[c, 3] for c in (0, 1, 3)]


def velocity64(ivp, cur, prev, depth, W, H, mutation=None, P=None):
    """Steps 2 and 3 of crychic_taa in float64: dict of vx, vy (pixels), a3, b3, b3_scale (the sum of the magnitudes of b[3]'s four
    terms) and `abnormal` (a float64 intermediate outside binary32's normal range).  P: (H, W, 3) world points to reproject in place
    of those of step 2."""
    with np.errstate(all="ignore"):
        h = P       # given points (the physical anchor's true ones) have no homogeneous stage to watch
        if P is None:
            P, h = world_point64(ivp, depth, W, H, mutation, parts=True)
        if mutation == "cur_prev_swapped":
            cur, prev = prev, cur
        a, b = project64(P, cur), project64(P, prev)
        hw = 0.5 * ((W - 1) if mutation == "hw_w_minus_1" else W)
        hh = 0.5 * H
        ra, rb = 1.0 / a[2], 1.0 / b[2]
        ax, bx, ay, by = a[0] * ra, b[0] * rb, a[1] * ra, b[1] * rb
        vx, vy = (ax - bx) * hw, (by - ay) * hh
        Mp = _columns(prev)
        scale = np.abs(P[..., 0] * Mp[3, 0]) + np.abs(P[..., 1] * Mp[3, 1]) + np.abs(P[..., 2] * Mp[3, 2]) + abs(Mp[3, 3])
        ab = _abnormal(*([h[..., c] for c in range(h.shape[-1])] + [P[..., c] for c in range(3)] + a + b + [ra, rb, ax, bx, ay, by, vx, vy]))
    return dict(vx=vx, vy=vy, a3=a[2], b3=b[2], b3_scale=scale, abnormal=ab, P=P)


# ---- motion blur ---------------------------------------------------------------------------------------------------------------------

def mb_scale64(vx, vy, a3, b3, shutter, R, mutation=None):
    """Step A from the velocity on: (s_x 16, s_y 16, valid), unrounded."""
    with np.errstate(all="ignore"):
        valid = (a3 > 0) & (b3 > 0) & (np.abs(vx) < np.inf) & (np.abs(vy) < np.inf)
        sh = shutter / (255.0 if mutation == "shutter_255" else 256.0)
        s_x, s_y = vx * sh, vy * sh
        m = np.hypot(s_x, s_y) if mutation == "euclid_clamp" else np.maximum(np.abs(s_x), np.abs(s_y))
        k = np.where(m > R, R / m, 1.0)
        s_x, s_y = s_x * k, s_y * k
        zero = np.zeros_like(vx)
    return np.where(valid, s_x * 16.0, zero), np.where(valid, s_y * 16.0, zero), valid


def mb_quantise(s16, R):
    """Step A.4: clamp(floor(s 16 + 0.5), -16 R, 16 R), int64."""
    with np.errstate(all="ignore"):
        q = np.floor(np.clip(s16, -16.0 * R - 8, 16.0 * R + 8) + 0.5)
    return np.clip(np.where(np.isfinite(q), q, 0.0), -16 * R, 16 * R).astype(np.int64)


def mb_step_a64(case, mutation=None):
    """Step A of a motion_blur_lib.Case: (qx, qy, abnormal), int64 planes in 1/16 pixel."""
    v = velocity64(case.ivp, case.cur, case.prev, case.depth, case.W, case.H, mutation)
    sx16, sy16, _ = mb_scale64(v["vx"], v["vy"], v["a3"], v["b3"], case.shutter, case.radius, mutation)
    with np.errstate(all="ignore"):
        ab = v["abnormal"] | _abnormal(sx16 / 16.0, sy16 / 16.0)
    return mb_quantise(sx16, case.radius), mb_quantise(sy16, case.radius), ab


def word_parts(words):
    """(qx, qy, len) of uint32 velocity words, int64: the two int16 fields and their Chebyshev norm."""
    w = np.asarray(words).astype(np.int64)
    qx, qy = w & 0xFFFF, (w >> 16) & 0xFFFF
    qx, qy = qx - ((qx & 0x8000) << 1), qy - ((qy & 0x8000) << 1)
    return qx, qy, np.maximum(np.abs(qx), np.abs(qy))


def _keys(words):
    return (word_parts(words)[2] << 32) | np.asarray(words).astype(np.int64)


def mb_tiles64(words, mutation=None):
    """Step A': the (ceil(H / 16), ceil(W / 16)) plane of the word of the largest key of every 16 x 16 tile."""
    H, W = words.shape
    th, tw = (H + 15) // 16, (W + 15) // 16
    key = np.full((th * 16, tw * 16), -1, np.int64)
    key[:H, :W] = _keys(words)
    t = key.reshape(th, 16, tw, 16).transpose(0, 2, 1, 3).reshape(th, tw, 256)
    if mutation == "tile_first_lane":       # the first lane in row-major order that has the largest length
        ln = np.where(t < 0, -1, t >> 32)
        pick = np.take_along_axis(t, ln.argmax(axis=2)[..., None], axis=2)[..., 0]
    else:
        pick = t.max(axis=2)
    return (pick & 0xFFFFFFFF).astype(np.uint32)


def mb_gather64(img, words, depths, tiles, N, row0=0, rows=None, mutation=None):
    """Step B for rows [row0, row0 + rows): the (rows, W, 4) uint8 frame from the velocity plane (words and depth fields) and the tile
    plane."""
    H, W = words.shape
    rows = H - row0 if rows is None else rows
    img = np.asarray(img).astype(np.int64)
    th, tw = tiles.shape
    key = np.full((th + 2, tw + 2), -1, np.int64)
    key[1:-1, 1:-1] = _keys(tiles)
    best = np.max([key[1 + j:1 + j + th, 1 + i:1 + i + tw] for j in (-1, 0, 1) for i in (-1, 0, 1)], axis=0)
    py, px = np.meshgrid(np.arange(row0, row0 + rows), np.arange(W), indexing="ij")
    vN = best[py >> 4, px >> 4] & 0xFFFFFFFF
    nx, ny, lenN = word_parts(vN)
    bayer = BAYER.T if mutation == "bayer_transposed" else BAYER
    b = bayer[py & 3, px & 3]
    _, _, lens = word_parts(words)
    dep = np.asarray(depths).astype(np.int64)
    dX, lenX = dep[py, px], lens[py, px]
    Wt = np.ones((rows, W), np.int64)
    S = img[py, px, :3].copy()
    for i in range(N):
        m = 16 * i + b - 8 * N
        ox, oy = (nx * m + 8 * N) // (16 * N), (ny * m + 8 * N) // (16 * N)
        dist = np.maximum(np.abs(ox), np.abs(oy))
        qx, qy = np.clip(px + ((ox + 8) >> 4), 0, W - 1), np.clip(py + ((oy + 8) >> 4), 0, H - 1)
        dY, lenY = dep[qy, qx], lens[qy, qx]
        near_y = (2 * dist < lenY) if mutation == "dist_strict" else (2 * dist <= lenY)
        w = ((dY <= dX) & near_y).astype(np.int64) + ((dY >= dX) & (2 * dist <= lenX)).astype(np.int64)
        Wt += w
        S += w[..., None] * img[qy, qx, :3]
    out = img[py, px].copy()
    blurred = (2 * S + Wt[..., None]) // (2 * Wt[..., None])
    out[..., :3] = np.where((lenN < 8)[..., None], out[..., :3], blurred)
    return out.astype(np.uint8)


# ---- temporal anti-aliasing -----------------------------------------------------------------------------------------------------------

TAA_RESET, TAA_NO_CLAMP = 1, 2
TAA_BOUND_MARGIN = 1.0 / 16.0     # of 1/256 texel
TAA_B3_MARGIN = 1.0e-4            # of the sum of the magnitudes of b[3]'s terms


def taa_front64(case, mutation=None):
    """Steps 2 - 4a of a taa_lib.Case: dict of fxp, fyp, b3, X, Y (int64 floors, 0 where not finite), has (the float64 history
    predicate) and decided."""
    W, H = case.W, case.H
    v = velocity64(case.ivp, case.cur, case.prev, case.depth, W, H, mutation)
    with np.errstate(all="ignore"):
        fxp = (np.arange(W, dtype=np.float64)[None, :] - v["vx"]) * 256.0
        fyp = (np.arange(H, dtype=np.float64)[:, None] - v["vy"]) * 256.0
        xmax = 256.0 * W if mutation == "xmax_256w" else (W - 1) * 256.0
        ymax = (H - 1) * 256.0
        b3 = v["b3"]
        front = (b3 >= 0) if mutation == "b3_ge" else (b3 > 0)
        has = front & (fxp >= 0) & (fxp <= xmax) & (fyp >= 0) & (fyp <= ymax)
        if case.flags & TAA_RESET:
            has = np.zeros_like(has)
        near_bound = np.zeros((H, W), bool)
        for f, top in ((fxp, (W - 1) * 256.0), (fyp, (H - 1) * 256.0)):
            near_bound |= ~np.isfinite(f) | (np.abs(f) <= TAA_BOUND_MARGIN) | (np.abs(f - top) <= TAA_BOUND_MARGIN)
        near_zero = ~(np.abs(b3) > TAA_B3_MARGIN * v["b3_scale"])
        still = (v["vx"] == 0) & (v["vy"] == 0)
        decided = still | ~(near_bound | near_zero)
        if case.flags & TAA_RESET:
            decided = np.ones_like(decided)
        X = np.where(np.isfinite(fxp), np.floor(np.clip(fxp, -1.0e9, 1.0e9)), 0.0).astype(np.int64)
        Y = np.where(np.isfinite(fyp), np.floor(np.clip(fyp, -1.0e9, 1.0e9)), 0.0).astype(np.int64)
    return dict(fxp=fxp, fyp=fyp, b3=b3, X=X, Y=Y, has=has, decided=decided, still=still)


def taa_back64(case, X, Y, has, row0=0, rows=None, mutation=None):
    """Steps 1 and 4b - 7 for rows [row0, row0 + rows) of a taa_lib.Case, from (H, W) integer history positions X, Y in 1/256 texel
    (clamped into the frame here) and the boolean plane `has`: ((rows, W, 4) uint8 out, (rows, W, 4) uint16 history_out)."""
    W, H = case.W, case.H
    rows = H - row0 if rows is None else rows
    img = case.img.astype(np.int64)
    ys = np.arange(row0, row0 + rows)
    c = img[ys]
    ylo, yhi = (row0, row0 + rows - 1) if mutation == "lohi_row_range" else (0, H - 1)
    nb = [img[np.clip(ys + j, ylo, yhi)][:, np.clip(np.arange(W) + i, 0, W - 1), :3] for j in (-1, 0, 1) for i in (-1, 0, 1)]
    lo, hi = 256 * np.min(nb, axis=0), 256 * np.max(nb, axis=0)
    n = 256 * c[..., :3]
    if case.hist is not None and not (case.flags & TAA_RESET):
        hist = case.hist.astype(np.int64)
        Xc, Yc = np.clip(X[ys], 0, (W - 1) * 256), np.clip(Y[ys], 0, (H - 1) * 256)
        xi, fx, yi, fy = Xc >> 8, (Xc & 255)[..., None], Yc >> 8, (Yc & 255)[..., None]
        x1, y1 = np.minimum(xi + 1, W - 1), np.minimum(yi + 1, H - 1)
        top = hist[yi, xi, :3] * (256 - fx) + hist[yi, x1, :3] * fx
        bot = hist[y1, xi, :3] * (256 - fx) + hist[y1, x1, :3] * fx
        hv = (top * (256 - fy) + bot * fy + (32767 if mutation == "round_32767" else 32768)) >> 16
        hc = hv if case.flags & TAA_NO_CLAMP else np.minimum(np.maximum(hv, lo), hi)
        wh, wc = (case.blend, 256 - case.blend) if mutation == "blend_swapped" else (256 - case.blend, case.blend)
        n = np.where(has[ys][..., None], (hc * wh + c[..., :3] * 256 * wc + 128) >> 8, n)
    hout = np.concatenate([n, 256 * c[..., 3:]], axis=-1).astype(np.uint16)
    out = np.concatenate([np.minimum((n + 128) >> 8, 255), c[..., 3:]], axis=-1).astype(np.uint8)
    return out, hout


def taa_candidates64(case, front, row0=0, rows=None, mutation=None):
    """[(out, history_out)] of the back end at (X + dx, Y + dy), dx, dy = -1 .. 1, all with history; and the pair without history."""
    W, H = case.W, case.H
    yes, no = np.ones((H, W), bool), np.zeros((H, W), bool)
    with_h = [taa_back64(case, front["X"] + dx, front["Y"] + dy, yes, row0, rows, mutation) for dy in (0, -1, 1) for dx in (0, -1, 1)]
    return with_h, taa_back64(case, front["X"], front["Y"], no, row0, rows, mutation)


# ---- depth of field --------------------------------------------------------------------------------------------------------------------

DOF_U_MARGIN = 1.0e-3


def dof_u64(frame, params):
    """The unrounded circle of confusion u of every texel of a dof_lib.Frame, in 1/16 pixel (NaN where the header's is)."""
    with np.errstate(all="ignore"):
        g = float(np.float32(params["focus"]) / np.float32(frame.B))            # a binary32 host constant
        ap16 = float(np.float32(params["aperture"]) * np.float32(16.0))
        d = (frame.depth.astype(np.int64) & 0xFFFFFF).astype(np.float64) / 16777215.0
        return np.abs(1.0 - (d - f32(frame.A)) * g) * ap16


def dof_c64(u, R):
    """c = (uint32_t)(clampf(u, 0, 16 R) + 0.5), a NaN giving 0; and the texels whose u + 0.5 lies within DOF_U_MARGIN of an integer
    inside the clamp's range."""
    with np.errstate(all="ignore"):
        cl = np.where(np.isnan(u), 0.0, np.minimum(np.maximum(u, 0.0), 16.0 * R))
        t = cl + 0.5
        marginal = (np.abs(t - np.round(t)) <= DOF_U_MARGIN) & ~np.isnan(u) & (u <= 16.0 * R + DOF_U_MARGIN)
    return np.floor(t).astype(np.int64), marginal


def dof_disc(R):
    return [(ox, oy) for oy in range(-R, R + 1) for ox in range(-R, R + 1) if ox * ox + oy * oy <= R * R]


def dof_tables(mutation=None):
    """(inv[0 .. 128], {offset: d16} of the radius-8 disc)."""
    inv = np.array([(1 << 20) // max(c, 15 if mutation == "inv_max_15" else 16) ** 2 for c in range(129)], np.int64)
    return inv, {o: math.isqrt(256 * (o[0] * o[0] + o[1] * o[1])) for o in dof_disc(8)}


def dof_back64(c, depth, img, R, row0=0, rows=None, mutation=None):
    """The gather for rows [row0, row0 + rows) from a (H, W) plane of circles of confusion: (rows, W, 4) uint8."""
    H, W = c.shape
    rows = H - row0 if rows is None else rows
    inv, d16 = dof_tables(mutation)
    c = np.asarray(c).astype(np.int64)
    D = np.asarray(depth).astype(np.int64) & 0xFFFFFF
    img = np.asarray(img).astype(np.int64)
    py, px = np.meshgrid(np.arange(row0, row0 + rows), np.arange(W), indexing="ij")
    cp, Dp = c[py, px], D[py, px]
    Sw = np.zeros((rows, W), np.int64)
    S = np.zeros((rows, W, 3), np.int64)
    y_lo, y_hi = (row0, row0 + rows) if mutation == "frame_is_row_range" else (0, H)
    for o in dof_disc(R):
        sx, sy = px + o[0], py + o[1]
        inside = (sx >= 0) & (sx < W) & (sy >= y_lo) & (sy < y_hi)
        qx, qy = np.clip(sx, 0, W - 1), np.clip(sy, 0, H - 1)
        cs, Ds = c[qy, qx], D[qy, qx]
        behind = (Ds >= Dp) if mutation == "ds_ge_dp" else (Ds > Dp)
        ce = np.where(behind, np.minimum(cs, cp), cs)
        k = np.clip(ce + (7 if mutation == "k_plus_7" else 8) - d16[o], 0, 16)
        w = np.where(inside, k * inv[ce], 0)
        Sw += w
        S += w[..., None] * img[qy, qx, :3]
    out = img[py, px].copy()
    Sw = np.maximum(Sw, 1)          # only a mutation can make it 0
    out[..., :3] = (S + (Sw >> 1)[..., None]) // Sw[..., None]
    return np.clip(out, 0, 255).astype(np.uint8)


def dof_marginal_discs(marginal, R):
    """The pixels whose disc, cut to the frame, holds a marginal texel."""
    H, W = marginal.shape
    pad = np.zeros((H + 2 * R, W + 2 * R), bool)
    pad[R:R + H, R:R + W] = marginal
    out = np.zeros((H, W), bool)
    for ox, oy in dof_disc(R):
        out |= pad[R + oy:R + oy + H, R + ox:R + ox + W]
    return out


# ---- volumetric fog --------------------------------------------------------------------------------------------------------------------

FOG_THRESHOLDS = (30.0, 50.0, 80.0, 100.0)
FOG_T_MARGIN = 1.0e-4             # relative, on the cascade thresholds
FOG_Z_MARGIN = 1.0e-5             # on s.z against the map
FOG_Q_MARGIN = 0.02               # on q 65536 + 0.5


def fog_texel_margin(dim):
    return 1.0e-3 + 4.0e-6 * dim


def fog64(frame, img, params, mutation=None):
    """crychic_fog over a fog_lib.Frame: (lo, hi, stats): the (H, W, 3) int64 bounds of R, G, B, and the counts of samples and of
    marginal samples.  S runs from the sure-lit samples to the sure-lit and the marginal ones; qi over floor(q 65536 + 0.5) and, where
    that argument lies within FOG_Q_MARGIN of an integer, its neighbour."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    N = int(params["steps"])
    dim = frame.dim
    with np.errstate(all="ignore"):
        invN = np.float32(1.0) / np.float32(N)
        cc = float(-(np.float32(params["density"]) * np.float32(1.44269504)) * invN)
        invN, maxd = float(invN), f32(params["maxDistance"])
        eye = frame.eye.astype(np.float64)
        ST = [_columns(frame.st[j]) for j in range(4)]
        a = np.array([[eye @ ST[j][c, :3] + ST[j][c, 3] for c in range(3)] for j in range(4)])         # (4, 3)
        P = world_point64(frame.ivp, frame.depth, W, H, mutation)
        r = P - eye
        L = np.sqrt(np.clip((r * r).sum(axis=-1), 2.0 ** -100, 2.0 ** 100))
        L = np.where(np.isnan(L), 2.0 ** -50, L)
        Lc = L if mutation == "lc_unclamped" else np.minimum(L, maxd)
        q = np.exp2(np.clip(cc * Lc, -125.0, 127.0))
        arg = q * 65536.0 + 0.5
        qi0 = np.floor(arg).astype(np.int64)
        cands = [(qi0, np.ones((H, W), bool)), (qi0 - 1, (arg - qi0 <= FOG_Q_MARGIN) & (qi0 > 0)),
                 (qi0 + 1, (qi0 + 1 - arg <= FOG_Q_MARGIN) & (qi0 < 65536))]
        stepLen = Lc * invN
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        jit = (BAYER[py & 3, px & 3] + (0.0 if mutation == "jit_no_half" else 0.5)) / 16.0
        invL = 1.0 / L
        b = np.stack([np.stack([r @ ST[j][c, :3] for c in range(3)], axis=-1) for j in range(4)])     # (4, H, W, 3)
        mapd = (frame.maps.astype(np.int64) & 0xFFFFFF).astype(np.float64) / 16777215.0
        tol = fog_texel_margin(dim)
        T = [np.full((H, W), 65536, np.int64) for _ in cands]
        S_lo = [np.zeros((H, W), np.int64) for _ in cands]
        S_hi = [np.zeros((H, W), np.int64) for _ in cands]
        n_marginal = 0
        for i in range(N):
            t = (i + jit) * stepLen
            if mutation == "cascade_le":
                j = (t > 30.0).astype(np.int64) + (t > 50.0) + (t > 80.0) + (t > 100.0)
            else:
                j = (t >= 30.0).astype(np.int64) + (t >= 50.0) + (t >= 80.0) + (t >= 100.0)
            marg = np.zeros((H, W), bool)
            for thr in FOG_THRESHOLDS:
                marg |= np.abs(t - thr) <= FOG_T_MARGIN * thr
            beyond = j == 4
            jj = np.minimum(j, 3)
            f = t * invL
            s = np.take_along_axis(b, jj[None, ..., None], axis=0)[0] * f[..., None] + a[jj]
            fx, fy = s[..., 0] * dim, s[..., 1] * dim
            clearly_out = (fx < -tol) | (fx > dim + tol) | (fy < -tol) | (fy > dim + tol) | np.isnan(fx) | np.isnan(fy)
            near_texel = (np.abs(fx - np.round(fx)) <= tol) | (np.abs(fy - np.round(fy)) <= tol)
            ix, iy = np.clip(np.floor(fx), 0, dim - 1), np.clip(np.floor(fy), 0, dim - 1)
            ix, iy = np.where(np.isnan(ix), 0, ix).astype(np.int64), np.where(np.isnan(iy), 0, iy).astype(np.int64)
            m = mapd[jj, iy, ix]
            lit_in = (s[..., 2] < m) if mutation == "sz_lt_map" else (s[..., 2] <= m)
            near_z = np.abs(s[..., 2] - m) <= FOG_Z_MARGIN
            lit = beyond | clearly_out | lit_in
            marg |= ~beyond & ~clearly_out & (near_texel | near_z)
            n_marginal += int(marg.sum())
            for k, (qi, _) in enumerate(cands):
                Tn = (T[k] * qi + (32767 if mutation == "t_round_32767" else 32768)) >> 16
                w = T[k] - Tn
                S_lo[k] += np.where(lit & ~marg, w, 0)
                S_hi[k] += np.where(lit | marg, w, 0)
                T[k] = Tn
        rgb = img[..., :3].astype(np.int64)
        amb = np.array(params["ambient"][:3], np.int64)
        sun = np.array(params["sun"][:3], np.int64)
        lo = np.full((H, W, 3), 1 << 40, np.int64)
        hi = np.full((H, W, 3), -1, np.int64)
        for k, (_, ok) in enumerate(cands):
            base = rgb * T[k][..., None] + amb * (65536 - T[k])[..., None] + 32768
            o_lo = np.minimum((base + sun * S_lo[k][..., None]) >> 16, 255)
            o_hi = np.minimum((base + sun * S_hi[k][..., None]) >> 16, 255)
            lo = np.where(ok[..., None], np.minimum(lo, o_lo), lo)
            hi = np.where(ok[..., None], np.maximum(hi, o_hi), hi)
    return lo, hi, dict(samples=N * H * W, marginal=n_marginal)
