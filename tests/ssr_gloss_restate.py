"""An int64 numpy restatement of crychic_ssr_pyramid and of step 6b of crychic_ssr_glossy (TEST INFRASTRUCTURE ONLY), written from the
definition in include/crychic_hip.h alone: whole arrays at a time, no code of csrc/ or of tests/ssr_gloss_ref.  It is all integer, so
it equals the checker on every byte, without margins."""
import numpy as np

MAX_LEVELS = 8


def level_sizes(W, H, levels):
    """[(W_k, H_k) for k = 0 .. n_eff]: levels counts level 0; the chain stops at the first 1 x 1 level."""
    assert W > 0 and H > 0 and 1 <= levels <= MAX_LEVELS
    sizes = [(W, H)]
    while len(sizes) < levels and sizes[-1] != (1, 1):
        w, h = sizes[-1]
        sizes.append(((w + 1) >> 1, (h + 1) >> 1))
    return sizes


def offsets(W, H, levels):
    """([byte offset of level k for k = 0 .. n_eff] (0 for level 0), the workspace's bytes): back to back, each on a 16-byte boundary."""
    off, at, end = [0], 0, 0
    for w, h in level_sizes(W, H, levels)[1:]:
        off.append(at)
        end = at + w * h * 4
        at = (end + 15) // 16 * 16
    return off, end


def downsample(src):
    """One level from the (h, w, 4) level `src`: (1, 3, 3, 1) x (1, 3, 3, 1) over columns 2x - 1 .. 2x + 2 and rows likewise, clamped."""
    s = src.astype(np.int64)
    h, w = s.shape[:2]
    wd, hd = (w + 1) >> 1, (h + 1) >> 1
    taps = (1, 3, 3, 1)
    xs = [np.clip(2 * np.arange(wd) - 1 + i, 0, w - 1) for i in range(4)]
    ys = [np.clip(2 * np.arange(hd) - 1 + j, 0, h - 1) for j in range(4)]
    rows = sum(t * s[:, x] for t, x in zip(taps, xs))               # (h, wd, 4)
    total = sum(t * rows[y] for t, y in zip(taps, ys))              # (hd, wd, 4)
    assert total.max() <= 64 * 255
    return ((total + 32) >> 6).astype(np.uint8)


def pyramid(img, levels):
    """[level 0 (the frame), level 1, .. level n_eff] as (H_k, W_k, 4) uint8 arrays."""
    out = [np.asarray(img, np.uint8)]
    for _ in level_sizes(img.shape[1], img.shape[0], levels)[1:]:
        out.append(downsample(out[-1]))
    return out


def workspace(img, levels, fill):
    """The workspace crychic_ssr_pyramid leaves, in a flat uint8 array of `fill` of at least 16 bytes."""
    off, end = offsets(img.shape[1], img.shape[0], levels)
    ws = np.full(max(end, 16), fill, np.uint8)
    for k, lv in enumerate(pyramid(img, levels)):
        if k:
            ws[off[k]:off[k] + lv.size] = lv.reshape(-1)
    return ws


def fetch(level, k, hx, hy):
    """fetch(k) of step 6b at the hit pixels (hx, hy) (int64 arrays): (n, 3) int64."""
    hk, wk = level.shape[:2]
    lv = level.astype(np.int64)

    def axis(h, n):
        U = np.maximum(((2 * h + 1) * 128) >> k, 128) - 128
        c0 = np.minimum(U >> 8, n - 1)
        return c0, np.minimum(c0 + 1, n - 1), (U & 255)[:, None]
    x0, x1, fx = axis(hx, wk)
    y0, y1, fy = axis(hy, hk)
    top = lv[y0, x0, :3] * (256 - fx) + lv[y0, x1, :3] * fx
    bot = lv[y1, x0, :3] * (256 - fx) + lv[y1, x1, :3] * fx
    return (top * (256 - fy) + bot * fy + 32768) >> 16


def hit_colour(levels_list, hx, hy, lq):
    """hit_c of step 6b for hit pixels (hx, hy) with level words lq (int64 arrays): (n, 3) int64."""
    n_eff = len(levels_list) - 1
    k, f = lq >> 8, lq & 255
    assert (lq >= 0).all() and (lq <= 256 * n_eff).all()
    out = np.zeros((len(hx), 3), np.int64)
    for lvl in range(n_eff + 1):
        m = k == lvl
        if not m.any():
            continue
        v = fetch(levels_list[lvl], lvl, hx[m], hy[m])
        fm = f[m][:, None]
        if (fm > 0).any():          # f > 0 only below n_eff
            u = fetch(levels_list[lvl + 1], lvl + 1, hx[m], hy[m])
            v = np.where(fm == 0, v, (v * (256 - fm) + u * fm + 128) >> 8)
        out[m] = v
    return out
