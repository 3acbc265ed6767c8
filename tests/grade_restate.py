"""A numpy restatement of crychic_grade's lookup (TEST INFRASTRUCTURE ONLY), written from the comment in include/crychic_hip.h in
int64 arithmetic over whole frames.  It imports nothing of the checker (tests/grade_ref), of the host build or of csrc: the
definition is all-integer, so the three must agree on every byte, and tests/test_grade_host.py holds them to that.

MUTATIONS are misreadings of that comment made on purpose; SURVIVOR is a reading the comment allows."""
import numpy as np

MUTATIONS = ("trilinear", "round_128", "no_clamp", "blue_fastest", "weights_swapped")
SURVIVOR = "tie_reorder"


def apply(img, lut, mutation=None):
    """The (H, W, 4) uint8 frame `img` through the table `lut`, an (N, N, N, 4) uint8 array indexed [blue][green][red]."""
    assert mutation is None or mutation in MUTATIONS or mutation == SURVIVOR
    N = lut.shape[0]
    table = np.ascontiguousarray(lut).reshape(-1, 4).astype(np.int64)     # entry (i, j, k) at i + N (j + N k)
    v = img.reshape(-1, 4)[:, :3].astype(np.int64)
    p = v * (N - 1)
    cell = p // 255
    if mutation != "no_clamp":          # the misreading leaves v = 255 in cell N - 1 and looks up vertices outside the table
        cell = np.minimum(cell, N - 2)
    f = p - 255 * cell
    strides = np.array([N * N, N, 1] if mutation == "blue_fastest" else [1, N, N * N], np.int64)
    base = cell @ strides
    if mutation == "trilinear":
        num = np.zeros((v.shape[0], 3), np.int64)
        for corner in range(8):
            bits = np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1], np.int64)
            w = np.prod(np.where(bits == 1, f, 255 - f), axis=1)
            num += w[:, None] * table[base + bits @ strides, :3]
        out = (num + 255 ** 3 // 2) // 255 ** 3
    else:
        # the axes by falling fraction; a stable sort keeps red before green before blue at a tie, the survivor the other way round
        if mutation == SURVIVOR:
            order = 2 - np.argsort(-f[:, ::-1], axis=1, kind="stable")
        else:
            order = np.argsort(-f, axis=1, kind="stable")
        fs = np.take_along_axis(f, order, axis=1)
        step = strides[order]
        f1, f2, f3 = fs[:, 0], fs[:, 1], fs[:, 2]
        v1 = base + step[:, 0]
        v2 = v1 + step[:, 1]
        v3 = base + strides.sum()
        w = [255 - f1, f1 - f2, f2 - f3, f3]
        if mutation == "weights_swapped":
            w[1], w[2] = w[2], w[1]
        num = sum(wk[:, None] * table[vk, :3] for wk, vk in zip(w, (base, v1, v2, v3)))
        out = (num + (128 if mutation == "round_128" else 127)) // 255
    res = np.empty_like(img)
    res.reshape(-1, 4)[:, :3] = out
    res[..., 3] = img[..., 3]
    return res
