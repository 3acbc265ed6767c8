"""Measures crychic_ssr_glossy's default coneScale (TEST INFRASTRUCTURE ONLY; CPU, the checker alone):

    python tests/ssr_gloss_quality.py > profiles/ssr_gloss_quality.txt

Scene: ssr_lib.mirror_scene at 128 x 96 with the floor at roughness rho; the wall carries a 4-pixel checker over its coordinate ramp.
Ground truth, per floor pixel: the mean over 256 GGX (a = rho) microfacet normals -- the same Hammersley set for every pixel -- of the
wall's colour where the view ray mirrored at that normal meets the wall, in float64; pixels with under 90 % of the rays landing on
the wall inside the frame are left out, as are pixels that are not mirror_eligible or for which the pass reports no hit.
Metric: the mean absolute error, over those pixels and R, G, B, of the colour the pass fetched (the checker's debug plane) against
that truth.  Grid: coneScale x rho; coneScale 0 is the sharp pass.  The default is the grid value with the lowest mean over rho; if no
grid value beats coneScale 0 at rho = 0.7 the default is 0.
A second table, for information only and never the source of the default, keeps the pixels with at least INFO_SHARE of their rays
landing and takes the mean over the rays that land: a lobe cut off at the frame's border, so a biased truth."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ssr_gloss_lib as gl      # noqa: E402
import ssr_lib as sl            # noqa: E402

W, H = 128, 96
CONES = (0.0, 0.25, 0.35, 0.5, 0.7, 1.0, 1.4, 2.0)
ROUGH = (0.3, 0.5, 0.7)
SAMPLES = 256
LEVELS = 6
RULE_SHARE, INFO_SHARE = 0.9, 0.2


def wall_colour(px, py):
    """The wall's colour at integer pixel coordinates: the ramp of ssr_lib.mirror_scene with a 4-pixel checker over it."""
    chk = ((px // 4 + py // 4) & 1).astype(np.int64)
    return np.stack([px + 96 * chk, py + 96 * chk, 0x40 + 128 * chk], axis=-1)


def hammersley(n):
    i = np.arange(n)
    v = np.zeros(n)
    f, k = 0.5, i.copy()
    while k.any():
        v += f * (k & 1)
        k >>= 1
        f *= 0.5
    return (i + 0.5) / n, v


def scene(rho):
    frame, img, truth = gl.anchor_scene(W, H, rough=rho)
    ys, xs = np.mgrid[0:H, 0:W]
    img = img.copy()
    wall = ~truth["floor"]
    img[wall, :3] = wall_colour(xs, ys)[wall].astype(np.uint8)
    return frame, img, truth


def ground_truth(rho, truth):
    """((H, W, 3) float64 mean colour, (H, W) share of the rays that land on the wall inside the frame) for the floor pixels."""
    from crychic_renderer_amd import scene as sc
    cam = sc.default_camera(W, H)
    ex, ey, ez = (float(v) for v in cam.pos)
    th, aspect = math.tan(0.5 * cam.fovY), float(cam.aspect)
    xs = (np.arange(W) + 0.5) / W * 2.0 - 1.0
    ys = 1.0 - (np.arange(H) + 0.5) / H * 2.0
    d = np.stack([np.broadcast_to((xs * aspect * th)[None, :], (H, W)), np.broadcast_to((ys * th)[:, None], (H, W)), np.ones((H, W))], axis=-1)
    floor = truth["floor"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(floor, -ey / d[..., 1], 1.0)
    P = np.array([ex, ey, ez]) + t[..., None] * d
    V = d / np.linalg.norm(d, axis=-1, keepdims=True)
    u1, u2 = hammersley(SAMPLES)
    a2 = rho * rho
    cos_t = np.sqrt((1.0 - u1) / (1.0 + (a2 - 1.0) * u1))
    sin_t = np.sqrt(1.0 - cos_t * cos_t)
    Hn = np.stack([sin_t * np.cos(2 * math.pi * u2), cos_t, sin_t * np.sin(2 * math.pi * u2)], axis=-1)      # about the normal (0, 1, 0)
    total = np.zeros((H, W, 3))
    landed = np.zeros((H, W))
    for h in Hn:
        L = V - 2.0 * (V @ h)[..., None] * h
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (sl.WALL_Z - P[..., 2]) / L[..., 2]
            Q = P + s[..., None] * L
            vz = Q[..., 2] - ez
            sx = (0.5 + 0.5 * (Q[..., 0] - ex) / (vz * aspect * th)) * W
            sy = (0.5 - 0.5 * (Q[..., 1] - ey) / (vz * th)) * H
        ok = floor & (L[..., 1] > 0) & (L[..., 2] > 0) & (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        px, py = np.where(ok, sx, 0).astype(np.int64), np.where(ok, sy, 0).astype(np.int64)
        total += np.where(ok[..., None], wall_colour(px, py), 0)
        landed += ok
    with np.errstate(divide="ignore", invalid="ignore"):
        return total / landed[..., None], landed / SAMPLES


def measure(min_share):
    table = np.full((len(CONES), len(ROUGH)), np.nan)
    counts = []
    p = sl.PARAM_SETS["mirror_n64"]
    for j, rho in enumerate(ROUGH):
        frame, img, truth = scene(rho)
        mean, share = ground_truth(rho, truth)
        sel = None
        for i, cone in enumerate(CONES):
            _, _, dbg = gl.checker(frame, img, p, dict(coneScale=cone, levels=LEVELS))
            if sel is None:
                sel = sl.mirror_eligible(truth, W, H, p) & (share >= min_share) & (dbg[..., 0] == sl.ST_HIT)
                counts.append(int(sel.sum()))
            if sel.any():
                table[i, j] = np.abs(dbg[..., 5:8][sel].astype(np.float64) - mean[sel]).mean()
    return table, counts


def show(table, counts, share):
    print("# pixels with at least %.0f %% of their rays landing on the wall inside the frame, per rho: %s" % (100 * share, ", ".join(str(c) for c in counts)))
    print("coneScale " + " ".join("rho=%.1f" % r for r in ROUGH) + "    mean")
    for cone, row in zip(CONES, table):
        print("%9.2f " % cone + " ".join("%7.2f" % v for v in row) + " %7.2f" % row.mean())


def main():
    print("# tests/ssr_gloss_quality.py: mean absolute error (0 .. 255) of the colour crychic_ssr_glossy fetched against the mean of %d GGX" % SAMPLES)
    print("# (a = rho) microfacet reflections in float64; the mirror scene at %d x %d, %d levels, PARAM_SETS[\"mirror_n64\"]" % (W, H, LEVELS))
    table, counts = measure(RULE_SHARE)
    show(table, counts, RULE_SHARE)
    beats = table[1:, -1] < table[0, -1]            # false for a NaN
    means = table.mean(axis=1)
    best = CONES[int(np.nanargmin(means))] if beats.any() else 0.0
    if not beats.any():
        print("# FINDING: no grid value beats coneScale 0 at rho = 0.7%s: the default coneScale is 0" % (
            " -- the rule leaves no pixel to measure: a GGX lobe with a = rho >= 0.3 sends more than 10 % of its rays outside a frame of this field of view"
            if counts[-1] == 0 else ""))
    else:
        print("# lowest mean: coneScale %.2f: the default" % best)
    print("#")
    print("# for information only, not the source of the default: the truth taken over the rays that land (a lobe cut off at the frame's border)")
    info, icounts = measure(INFO_SHARE)
    show(info, icounts, INFO_SHARE)
    return best


if __name__ == "__main__":
    main()
