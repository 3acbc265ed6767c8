"""A numpy restatement of crychic_sharpen (TEST INFRASTRUCTURE ONLY), written from the comment in include/crychic_hip.h in int64
arithmetic over whole frames.  It imports nothing of the checker (tests/sharpen_ref), of the host build or of csrc: the definition
is all-integer, so the three must agree on every byte, and tests/test_sharpen_host.py holds them to that.  On every case it runs
unmutated it asserts what lets the definition go without a clamp: no numerator below 0, no output above 255.

MUTATIONS are misreadings of that comment made on purpose."""
import numpy as np

MUTATIONS = ("centre_left_out", "max_across_channels", "division_rounded", "clamp_to_rows", "shift_as_div_255")


def apply(img, strength=256, limit=3072, row0=0, rows=None, mutation=None):
    """Rows [row0, row0 + rows) of the (H, W, 4) uint8 frame `img` sharpened: a (rows, W, 4) uint8 array."""
    assert mutation is None or mutation in MUTATIONS
    H, W = img.shape[:2]
    rows = H - row0 if rows is None else rows
    px = img.astype(np.int64)
    ys = np.arange(row0, row0 + rows)
    xs = np.arange(W)
    lo_y, hi_y = (row0, row0 + rows - 1) if mutation == "clamp_to_rows" else (0, H - 1)
    e = px[ys]
    b = px[np.clip(ys - 1, lo_y, hi_y)]
    h = px[np.clip(ys + 1, lo_y, hi_y)]
    d = e[:, np.clip(xs - 1, 0, W - 1)]
    f = e[:, np.clip(xs + 1, 0, W - 1)]
    ring = [b, d, f, h]
    taps = ring if mutation == "centre_left_out" else ring + [e]
    mn = np.minimum.reduce(taps)[..., :3]
    mx = np.maximum.reduce(taps)[..., :3]

    def div(n, m):
        m1 = np.maximum(m, 1)
        return (n + m1 // 2) // m1 if mutation == "division_rounded" else n // m1
    q_lo = np.where(mx == 0, 0, div(mn << 12, mx))
    q_hi = np.where(mn == 255, 0, div((255 - mx) << 12, 255 - mn))
    q = np.minimum(q_lo, q_hi)
    a = np.minimum(q.max(axis=-1) if mutation == "max_across_channels" else q.min(axis=-1), limit)
    t = a * strength // 255 if mutation == "shift_as_div_255" else (a * strength) >> 8
    S = sum(r[..., :3] for r in ring)
    num = 16384 * e[..., :3] - t[..., None] * S
    den = 4 * (4096 - t)[..., None]
    out = (num + den // 2) // den
    if mutation is None:
        assert (num >= 0).all() and (out <= 255).all(), "the definition needs a clamp after all"
    res = np.empty((rows, W, 4), np.uint8)
    res[..., :3] = np.clip(out, 0, 255)
    res[..., 3] = e[..., 3]
    return res
