"""Triangle soups for the producer passes: small generated cases aimed at the rasteriser's own machinery -- the
batch lookup of the setup kernel, draw-order serials as the depth tie-break, the small / large split of the live list, the clears,
fp64 depth on steep slivers and clipped primitives in every pass.  Deterministic by seed, numpy only (`clip` and `mixed` take their
perspective camera from crychic_renderer_amd.scene.Constants).

A case is a dict: items (5-tuples (vertices, indices, instances, startIndexLocation, baseVertexLocation), see
oracle_lib.draw_item_fields), materials, textures (None or a list), view / viewproj (16 floats, as PassConstants stores them), W, H,
shadow_dim (the side of the square target the shadow pass of this case renders to) and case-specific notes for the host tier.

Target sizes are bounded by area: no frame has more pixels than 130 x 70, no shadow map more than 96 x 96.  Some cases need one
long axis: a pixel box of exactly 2049 = 3 * 683 pixels exists only in a target 683 pixels long."""
import numpy as np

from oracle_lib import INSTANCE_DT, MATERIAL_DT, VERTEX_DT

IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)
LARGE_BOX = 2048                    # raster.hip kLargeBox: a pixel box above this area gets a workgroup
MIXED_SIZES = ((130, 70), (97, 61), (66, 34), (16, 200), (200, 6))
MAX_FRAME_PIXELS, MAX_SHADOW_DIM, MAX_TRIANGLES = 130 * 70, 96, 3000


# ---- small pieces ---------------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sphere_normals(n):
    """n well separated unit vectors (a Fibonacci sphere): neighbours are about sqrt(4 pi / n) apart."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    r = np.sqrt(1.0 - z * z)
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def tangent_for(n):
    """A unit tangent perpendicular to each normal."""
    n = np.asarray(n, np.float64).reshape(-1, 3)
    axis = np.eye(3)[np.argmin(np.abs(n), axis=1)]
    return unit(np.cross(n, axis))


def flat_triangles(pos, normals, rng):
    """Three unshared vertices per triangle, all with the triangle's own normal: pos (n, 3, 3), normals (n, 3)."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3, 3)
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
    assert len(pos) == len(normals)
    v = np.zeros(len(pos) * 3, VERTEX_DT)
    v["Pos"] = pos.reshape(-1, 3)
    v["Normal"] = np.repeat(normals, 3, axis=0)
    v["TangentU"] = np.repeat(tangent_for(normals), 3, axis=0)
    v["TexC"] = rng.random((len(v), 2))
    return v


def translation(t):
    """World matrix of a translation in the transposed layout the instance records hold."""
    m = np.eye(4, dtype=np.float64)
    m[:3, 3] = t
    return m.astype(np.float32).reshape(-1)


def make_instances(worlds, material_indices):
    inst = np.zeros(len(worlds), INSTANCE_DT)
    inst["World"] = np.asarray(worlds, np.float32).reshape(len(worlds), 16)
    inst["TexTransform"] = IDENTITY
    inst["MaterialIndex"] = material_indices
    return inst


def make_materials(n):
    """n materials without textures, each with its own albedo (exact in fp32, so G1 names the instance that won a pixel)."""
    m = np.zeros(n, MATERIAL_DT)
    k = np.arange(n)
    m["DiffuseAlbedo"] = np.stack([(k + 1) / 512.0, ((7 * k + 3) % 509) / 512.0, ((13 * k + 5) % 503) / 512.0, np.ones(n)], axis=1)
    m["FresnelR0"] = 0.1
    m["Roughness"] = 0.25 + (k % 5) / 8.0
    m["Metalness"] = (k % 3) / 4.0
    m["MatTransform"] = IDENTITY
    m["DiffuseMapIndex"] = 0
    m["NormalMapIndex"] = 1
    return m


def px_to_ndc(p, W, H):
    """Pixel coordinates (y down, pixel k spans [k, k + 1)) -> NDC x, y."""
    p = np.asarray(p, np.float64)
    return np.stack([2.0 * p[..., 0] / W - 1.0, 1.0 - 2.0 * p[..., 1] / H], axis=-1)


def area2(p):
    """Twice the signed area of triangles (..., 3, 2) in screen coordinates; > 0 is clockwise on a y-down screen: front."""
    a, b, c = p[..., 0, :], p[..., 1, :], p[..., 2, :]
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])


def facing(p, front=True):
    """The triangles (n, 3, k) with vertices 1 and 2 swapped where needed so that all face the camera (or all away)."""
    p = np.array(p, np.float64)
    flip = (area2(p[..., :2]) > 0) != front
    p[flip] = p[flip][:, [0, 2, 1]]
    return p


def snap(ndc_xy, W, H):
    """24.8 screen coordinates of NDC positions with w = 1, in setup_triangle's own fp32 arithmetic."""
    f = np.float32
    x, y = np.asarray(ndc_xy[..., 0], f), np.asarray(ndc_xy[..., 1], f)
    sx = (x + f(1.0)) * (f(0.5) * f(W))
    sy = (f(1.0) - y) * (f(0.5) * f(H))
    return (np.floor(sx * f(256.0) + f(0.5)).astype(np.int64), np.floor(sy * f(256.0) + f(0.5)).astype(np.int64))


def pixel_box_area(X, Y, W, H):
    """Area of triangle_box for snapped vertices X, Y (..., 3): the pixels whose centres lie inside the bounding box and the target."""
    x0 = np.maximum((X.min(-1) - 128 + 255) >> 8, 0); x1 = np.minimum((X.max(-1) - 128) >> 8, W - 1)
    y0 = np.maximum((Y.min(-1) - 128 + 255) >> 8, 0); y1 = np.minimum((Y.max(-1) - 128) >> 8, H - 1)
    return np.where((x0 <= x1) & (y0 <= y1), (x1 - x0 + 1) * (y1 - y0 + 1), 0)


def covers(X, Y, W, H):
    """Coverage mask (H, W) of one snapped clockwise triangle: exact integer edge functions at the pixel centres, top-left rule."""
    cy, cx = np.mgrid[0:H, 0:W].astype(np.int64) * 256 + 128
    ok = np.ones((H, W), bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):
        w = (X[b] - X[a]) * (cy - Y[a]) - (Y[b] - Y[a]) * (cx - X[a])
        top_left = (Y[b] < Y[a]) or (Y[b] == Y[a] and X[b] > X[a])
        ok &= (w > 0) | ((w == 0) & top_left)
    return ok


def box_mips(level0):
    """A mip chain down to 1 x 1 by 2 x 2 box filtering of a square power-of-two RGBA8 image."""
    levels = [np.ascontiguousarray(level0)]
    while levels[-1].shape[0] > 1:
        a = levels[-1].astype(np.uint32)
        levels.append(((a[0::2, 0::2] + a[1::2, 0::2] + a[0::2, 1::2] + a[1::2, 1::2] + 2) // 4).astype(np.uint8))
    return levels


def pattern_textures(size=32):
    """A mipped diffuse map (index 0) and a mipped normal map with gentle bumps (index 1)."""
    y, x = np.mgrid[0:size, 0:size]
    d = np.zeros((size, size, 4), np.uint8)
    d[..., 0] = 40 + 6 * x; d[..., 1] = 250 - 5 * y; d[..., 2] = np.where((x // 4 + y // 4) % 2, 230, 60); d[..., 3] = 255
    n = np.zeros((size, size, 4), np.uint8)
    n[..., 0] = 128 + (20 * np.sin(2 * np.pi * x / 8.0)).astype(np.int32); n[..., 1] = 128 + (20 * np.cos(2 * np.pi * y / 8.0)).astype(np.int32)
    n[..., 2] = 250; n[..., 3] = 255
    return [box_mips(d), box_mips(n)]


# ---- packing groups of triangles into draw items over one vertex and one index buffer ---------------------------------------
BASES = (0, 5, -7, 1, -1, 12, -13, 3)     # baseVertexLocation of consecutive non-empty items
PAD = 32                                  # spare vertices at both ends of the vertex buffer, more than any two bases differ by

NO_INDICES, NO_INSTANCES = "no indices", "no instances"     # the two kinds of empty item


def pack(groups, rng):
    """groups: dicts with "v" (vertices, three per triangle) and "inst" (instance records), or NO_INDICES / NO_INSTANCES for an
    empty item.  All items share one vertex buffer (the groups' vertices, each group shuffled, between PAD spare vertices at each
    end) and one index buffer (three spare indices first).  Item k draws its own range of the index buffer through a non-zero
    startIndexLocation, and its indices are stored minus its baseVertexLocation (BASES in turn, both signs).  Every item's
    vertexCount is the whole buffer, and the spare vertices are copies of drawn ones, so a location that is off by one, or taken
    from a neighbouring item, reads a different but valid vertex and draws a wrong triangle instead of raising the bad-index flag.
    An empty item is either an item of no indices (a live instance, startIndexLocation at the end of its view) or one of no
    instances with null vertex and instance buffers."""
    real = [g for g in groups if isinstance(g, dict)]
    every = np.concatenate([g["v"] for g in real])
    spare = every[rng.integers(0, len(every), 2 * PAD)].copy()
    spare["Normal"] = (0.0, 0.0, 1.0); spare["TangentU"] = (1.0, 0.0, 0.0)
    vparts, iparts, off, pos = [spare[:PAD]], [np.full(3, PAD // 2, np.int64)], PAD, 3
    plan, nreal = [], 0
    for g in groups:
        if g == NO_INSTANCES:
            iparts.append(np.full(6, PAD // 2, np.int64))
            plan.append((NO_INSTANCES, pos, pos + 6, 0, None)); pos += 6
            continue
        if g == NO_INDICES:
            plan.append((NO_INDICES, pos, pos, BASES[nreal % len(BASES)], make_instances([IDENTITY], [0])))
            continue
        n = len(g["v"])
        perm = rng.permutation(n)
        inv = np.argsort(perm)
        base = BASES[nreal % len(BASES)]; nreal += 1
        vparts.append(g["v"][perm])
        iparts.append(off + inv - base)
        plan.append(("", pos, pos + n, base, g["inst"]))
        off += n; pos += n
    vparts.append(spare[PAD:]); iparts.append(np.full(3, PAD // 2, np.int64))
    ib = np.concatenate(iparts)
    assert ib.min() >= 0
    vb, ib = np.concatenate(vparts), ib.astype(np.uint32)
    items = []
    for kind, start, end, base, inst in plan:
        items.append((None, ib[:end], None, start, 0) if kind == NO_INSTANCES else (vb, ib[:end], inst, start, base))
    return items


def item_counts(items):
    """(indexCount, instanceCount) of every item."""
    return [((len(it[1]) if it[1] is not None else 0) - it[3], len(it[2]) if it[2] is not None else 0) for it in items]


def input_triangles(items):
    return sum((n // 3) * m for n, m in item_counts(items))


def finish(case):
    W, H = case["W"], case["H"]
    assert W * H <= MAX_FRAME_PIXELS and case["shadow_dim"] <= MAX_SHADOW_DIM and input_triangles(case["items"]) <= MAX_TRIANGLES
    case.setdefault("textures", None)
    for k in ("view", "viewproj"):
        case[k] = np.ascontiguousarray(case[k], np.float32).reshape(16)
    for it in case["items"]:
        if it[0] is not None:       # unit normals and tangents, never parallel: no plane of the oracle can hold a NaN
            n, t = it[0]["Normal"].astype(np.float64), it[0]["TangentU"].astype(np.float64)
            assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6) and np.allclose(np.linalg.norm(t, axis=1), 1.0, atol=1e-6)
            assert np.abs((n * t).sum(axis=1)).max() < 0.95
    return case


# ---- case `stack`: exact depth ties, decided by draw order ------------------------------------------------------------------
STACK_ITEMS, STACK_NO_INDICES, STACK_NO_INSTANCES = 19, 3, 8
STACK_INSTANCED = (1, 5, 10, 14, 17)
STACK_SHIFTS = ((0, 0), (896, -512), (-1344, 1024))     # instance translations in 1/256 pixel: copies of an item overlap each other


def stack(leading_empties=False, seed=7):
    """Identity View / ViewProj, positions in NDC on the 1/256-pixel grid, every vertex at z = 0.5: every overlap is an exact D24
    tie and the earliest primitive in draw order owns the pixel.  19 items (3 and 8 empty), several with three overlapping
    instances; each triangle has its own flat normal, each instance its own material.  The last triangle of every item is an exact
    copy of the first triangle of the previous non-empty item (with a normal of its own), so duplicates straddle every boundary
    between setup batches wherever the boundaries fall.  leading_empties: eight more empty items first.
    The launcher drops empty items on the host while it fills a batch, so they never reach the setup kernel's lookup: the 17 drawn
    items make setup launches of 8 + 8 + 1, and what the empty ones test is that dropping, null buffers included, and the slot
    numbering carried past them.
    case["prims"]: (X, Y, normal id, material) of every primitive in draw order, X, Y the expected snapped vertices."""
    W, H = 72, 40
    rng = np.random.default_rng(seed)
    normals = sphere_normals(256)[rng.permutation(256)]
    groups, prims, nn, nm, prev = [], [], 0, 0, None
    if leading_empties:
        groups += [NO_INDICES, NO_INSTANCES] * 4
    for k in range(STACK_ITEMS):
        if k in (STACK_NO_INDICES, STACK_NO_INSTANCES):
            groups.append(NO_INDICES if k == STACK_NO_INDICES else NO_INSTANCES)
            continue
        nt = int(rng.integers(3, 7))
        centre = np.stack([rng.integers(12 * 256, (W - 12) * 256, nt), rng.integers(8 * 256, (H - 8) * 256, nt)], axis=1)
        tri = centre[:, None, :] + rng.integers(-14 * 256, 14 * 256, (nt, 3, 2))
        tri = tri[np.abs(area2(tri)) > 30 * 65536]                    # no slivers here: ties are the subject
        tri = facing(tri).astype(np.int64)
        if prev is not None:
            tri = np.concatenate([tri, prev[None]])
        prev = tri[0]
        shifts = STACK_SHIFTS if k in STACK_INSTANCED else STACK_SHIFTS[:1]
        ids = np.arange(nn, nn + len(tri)); nn += len(tri)
        pos = np.concatenate([px_to_ndc(tri / 256.0, W, H), np.full((len(tri), 3, 1), 0.5)], axis=2)
        worlds = [translation((2.0 * sx / 256.0 / W, -2.0 * sy / 256.0 / H, 0.0)) for sx, sy in shifts]
        groups.append({"v": flat_triangles(pos, normals[ids], rng), "inst": make_instances(worlds, np.arange(nm, nm + len(shifts)))})
        for j, (sx, sy) in enumerate(shifts):
            prims += [(t[:, 0] + sx, t[:, 1] + sy, int(i), nm + j) for t, i in zip(tri, ids)]
        nm += len(shifts)
    assert nn <= len(normals)
    return finish({"name": "stack", "items": pack(groups, rng), "materials": make_materials(nm), "view": IDENTITY, "viewproj": IDENTITY,
                   "W": W, "H": H, "shadow_dim": 40, "prims": prims, "normals": normals})


def stack_winners(case, order=None):
    """The expected owner of every pixel of `stack`, restated in numpy: index into case["prims"] of the first primitive in draw
    order whose exact integer coverage holds the pixel centre, -1 where there is none.  Also returns how many primitives cover it."""
    W, H = case["W"], case["H"]
    win = np.full((H, W), -1, np.int64)
    count = np.zeros((H, W), np.int64)
    for k in (range(len(case["prims"])) if order is None else order):
        X, Y = case["prims"][k][:2]
        c = covers(X, Y, W, H)
        win[c & (win < 0)] = k
        count += c
    return win, count


def reversed_items(case):
    out = dict(case)
    out["items"] = case["items"][::-1]
    return out


# ---- case `threshold`: the small / large split of the live list -------------------------------------------------------------
# variant: (W, H, shadow_dim, pixel boxes (w, h) to fill).  Areas 2047 = 89 x 23, 2048, 2049 = 683 x 3, 2050 and 2080 sit on both
# sides of the split; the large ones have heights 13, 17, 22, 31, 33 and widths 15, 17, 63, 65, 70: no multiples of the 16 x 4 footprint.
THRESHOLD = {
    "square": (95, 95, 95, ((64, 32), (65, 32), (89, 23), (41, 50), (32, 64), (23, 89), (95, 22), (95, 95), (63, 33), (17, 5), (5, 3))),
    "wide": (130, 70, 70, ((64, 32), (65, 32), (89, 23), (41, 50), (125, 17), (70, 31), (63, 33), (130, 1), (17, 5), (3, 70))),
    "long": (700, 13, 96, ((683, 3), (512, 4), (520, 4), (160, 13), (683, 2), (700, 1), (700, 13), (15, 13), (256, 8))),
    "tall": (17, 535, 96, ((15, 137), (15, 136), (17, 121), (17, 120), (1, 535), (4, 512), (3, 535), (17, 33), (16, 128))),
}


def threshold(variant="wide", seed=11):
    """Right triangles and thin diagonal slivers whose snapped pixel boxes have exactly the listed sizes, at random places, with a
    random z in [0, 1] per vertex (steep depth slopes), plus one-pixel-wide slivers along the whole target.
    case["box_areas"]: the pixel-box area of every triangle, computed with the rasteriser's own snapping."""
    W, H, sdim, boxes = THRESHOLD[variant]
    rng = np.random.default_rng(seed)
    tri = []
    for bw, bh in boxes:
        ox, oy = int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1))
        x1, y1 = ox + bw, oy + bh
        corners = [((ox, oy), (x1, oy), (ox, y1)), ((x1, y1), (ox, y1), (x1, oy))]           # the two right triangles of the box
        slivers = [((ox, oy), (x1, y1), (max(x1 - 1.5, ox), y1)), ((ox, y1), (x1, oy), (x1, min(oy + 1.25, y1)))]
        tri += [corners[int(rng.integers(0, 2))]] + slivers
    tri += [((0, 0), (W, H), (W, H - 1.0)), ((0, H), (W, 0), (1.0, H))]       # one pixel wide, from corner to corner
    tri = facing(np.array(tri, np.float64))
    n = len(tri)
    pos = np.concatenate([px_to_ndc(tri, W, H), rng.random((n, 3, 1))], axis=2)
    normals = sphere_normals(n)[rng.permutation(n)]
    v = flat_triangles(pos, normals, rng)
    X, Y = snap(v["Pos"].reshape(n, 3, 3), W, H)
    areas = pixel_box_area(X, Y, W, H)
    assert (areas > LARGE_BOX).any() and ((areas > 0) & (areas <= LARGE_BOX)).any(), "both classes of the live list"
    assert (areas == 2048).any() and (variant != "long" or (areas == 2049).any())
    order = rng.permutation(n)
    cut = sorted(rng.choice(np.arange(1, n), 3, replace=False))
    groups = [{"v": v.reshape(n, 3)[order[a:b]].reshape(-1), "inst": make_instances([IDENTITY], [g])}
              for g, (a, b) in enumerate(zip([0] + cut, cut + [n]))]
    return finish({"name": "threshold-" + variant, "items": pack(groups, rng), "materials": make_materials(len(groups)), "view": IDENTITY,
                   "viewproj": IDENTITY, "W": W, "H": H, "shadow_dim": sdim, "box_areas": areas})


# ---- case `grid`: the fill rule on a partition of the target ----------------------------------------------------------------
def grid(seed=3, W=97, H=61, nx=12, ny=8):
    """A triangulation of the whole target over a jittered lattice on the 1/256-pixel grid: some points exactly on pixel centres, one
    lattice row exactly horizontal and one column exactly vertical through pixel centres; all triangles front-facing at z = 0.5, each
    with its own flat normal.  Every pixel centre belongs to exactly one triangle under the top-left rule."""
    rng = np.random.default_rng(seed)
    gx = np.round(np.arange(nx + 1) * (W * 256.0 / nx)).astype(np.int64)
    gy = np.round(np.arange(ny + 1) * (H * 256.0 / ny)).astype(np.int64)
    X = np.repeat(gx[None, :], ny + 1, axis=0) + rng.integers(-int(0.22 * 256 * W / nx), int(0.22 * 256 * W / nx), (ny + 1, nx + 1))
    Y = np.repeat(gy[:, None], nx + 1, axis=1) + rng.integers(-int(0.22 * 256 * H / ny), int(0.22 * 256 * H / ny), (ny + 1, nx + 1))
    centre = rng.random((ny + 1, nx + 1)) < 0.2                     # exactly on a pixel centre
    X[centre] = (X[centre] >> 8) * 256 + 128; Y[centre] = (Y[centre] >> 8) * 256 + 128
    Y[3, :] = (gy[3] >> 8) * 256 + 128                              # a horizontal chain of edges through pixel centres
    X[:, 5] = (gx[5] >> 8) * 256 + 128                              # and a vertical one
    X[:, 0], X[:, -1], Y[0, :], Y[-1, :] = 0, W * 256, 0, H * 256   # the border of the target
    tri = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = [(X[q], Y[q]) for q in ((j, i), (j, i + 1), (j + 1, i + 1), (j + 1, i))]     # clockwise on screen
            tri += [(a, b, c), (a, c, d)] if rng.random() < 0.5 else [(a, b, d), (b, c, d)]
    tri = np.array(tri, np.int64)
    assert (area2(tri) > 0).all()
    n = len(tri)
    pos = np.concatenate([px_to_ndc(tri / 256.0, W, H), np.full((n, 3, 1), 0.5)], axis=2)
    v = flat_triangles(pos, sphere_normals(n)[rng.permutation(n)], rng)
    sx, sy = snap(v["Pos"].reshape(n, 3, 3), W, H)
    assert np.array_equal(sx, tri[..., 0]) and np.array_equal(sy, tri[..., 1])        # the pipeline's snap lands on the lattice
    return finish({"name": "grid", "items": [(v, np.arange(3 * n, dtype=np.uint32), make_instances([IDENTITY], [0]), 0, 0)],
                   "materials": make_materials(1), "view": IDENTITY, "viewproj": IDENTITY, "W": W, "H": H, "shadow_dim": 61, "triangles": n})


def permuted(case, seed):
    """`grid` with its triangles drawn in another order."""
    v, idx, inst = case["items"][0][:3]
    order = np.random.default_rng(seed).permutation(len(idx) // 3)
    out = dict(case)
    out["items"] = [(v, np.ascontiguousarray(idx.reshape(-1, 3)[order].reshape(-1)), inst, 0, 0)]
    return out


# ---- case `clip`: near, far and guard-band clipping under the perspective camera --------------------------------------------
def camera(W, H):
    """(View, ViewProj) of scene.Constants' camera: the eye at (0, 2, -15) looking down +z, 45 degrees, near 1, far 100."""
    from crychic_renderer_amd import scene
    cb = scene.Constants(W, H, 64).pass_cb
    return np.array(cb.View, np.float32), np.array(cb.ViewProj, np.float32)


TAN_HALF_FOV = np.tan(np.pi / 8.0)
EYE = np.array([0.0, 2.0, -15.0])


def from_view(p):
    """World position of a point given in view space (x right, y up, z = distance along the view direction)."""
    return np.asarray(p, np.float64) + EYE


def from_ndc(x, y, zv, W, H):
    """World position of the point seen at NDC (x, y) at view depth zv > 0."""
    return from_view([x * zv * TAN_HALF_FOV * W / H, y * zv * TAN_HALF_FOV, zv])


def clip_triangles(W, H):
    """The clipping subjects as world-space triangles, named.  Each is later drawn in both windings, so every one also contributes
    a back-facing triangle."""
    g = 2097152.0 / (0.5 * W) * TAN_HALF_FOV * W / H          # the guard band's slope in view space: |x| <= g z
    P = lambda x, y, zv: from_ndc(x, y, zv, W, H)
    t = {}
    t["near"] = [P(-0.5, -0.5, 5.0), P(0.1, 0.7, 8.0), from_view([1.0, -1.0, 0.3])]
    t["near2"] = [from_view([-0.6, 0.2, 0.5]), from_view([0.5, 0.4, 0.2]), P(0.3, -0.8, 12.0)]      # two vertices in front of the near plane
    t["far"] = [P(-0.8, 0.2, 50.0), P(0.6, 0.9, 80.0), P(0.2, -0.3, 150.0)]
    t["far2"] = [P(-0.2, 0.5, 400.0), P(0.9, 0.1, 120.0), P(0.4, 0.8, 60.0)]
    t["behind"] = [P(-0.7, -0.6, 6.0), P(-0.1, -0.2, 6.0), from_view([2.0, 1.0, -4.0])]             # w < 0
    t["behind2"] = [from_view([-3.0, -1.0, -2.0]), from_view([3.0, -2.0, -6.0]), P(0.0, 0.3, 20.0)]
    t["out1"] = [P(-0.5, -0.5, 10.0), P(-0.5, 0.5, 10.0), P(1.0e6, -0.5, 10.0)]                     # one vertex 10^6 NDC units out
    t["out2"] = [P(-1.0e6, 0.2, 20.0), P(0.0, -0.6, 20.0), P(0.3, 1.0e6, 20.0)]                     # two
    t["out3"] = [P(-1.0e6, -0.9, 30.0), P(0.0, 2.0e6, 30.0), P(1.0e6, -0.9, 30.0)]                  # three, the viewport inside
    t["near+band"] = [from_view([-3.0e6, -1.2, -1.0]), from_view([0.0, -1.2, 30.0]), from_view([3.0e6, -1.2, -1.0])]
    # a ground triangle whose three edges each cut a corner off the visible trapezoid (near and far plane, left and right band):
    # a heptagon, five fan triangles
    a = (-0.5 * g, 1.0), (-50.0 * g, 50.0), (0.5 * g, 1.0), (50.0 * g, 50.0), (75.0 * g, 75.0), (40.0 * g, 100.0)

    def meet(p, q, r, s):
        d1, d2 = np.subtract(q, p), np.subtract(s, r)
        u = np.linalg.solve(np.array([d1, -d2]).T, np.subtract(r, p))[0]
        return np.add(p, u * d1)
    corners = [meet(a[0], a[1], a[2], a[3]), meet(a[2], a[3], a[4], a[5]), meet(a[4], a[5], a[0], a[1])]
    t["heptagon"] = [from_view([x, -1.5, z]) for x, z in corners]
    t["heptagon2"] = [from_view([-x, 1.1 + 0.0004 * z, z]) for x, z in corners]                     # mirrored, above the eye, sloping
    t["outside"] = [P(3.0e5, -0.5, 10.0), P(3.0e5, 0.5, 10.0), P(4.0e5, 0.0, 10.0)]                 # wholly outside, right of the band
    t["outside2"] = [P(-3.0, 0.2, 9.0), P(-2.0, 0.7, 9.0), P(-2.5, -0.4, 7.0)]                      # outside the viewport, inside the band
    t["collinear"] = [P(-0.4, -0.4, 10.0), P(0.0, 0.0, 10.0), P(0.4, 0.4, 10.0)]
    t["two equal"] = [P(0.3, 0.3, 9.0), P(0.3, 0.3, 9.0), P(-0.2, 0.5, 9.0)]
    c = np.array([10.1, 10.1])
    for k, d in enumerate(([(0, 0), (0.3, 0), (0, 0.3)], [(0.55, 0.55), (0.8, 0.6), (0.6, 0.85)])):  # inside one pixel, off its centre
        t["subpixel%d" % k] = [P(*px_to_ndc(c + np.array(q), W, H), 7.0) for q in d]
    return t


CLIP_FANS = ("heptagon", "heptagon2")


def smooth_vertices(pos, rng):
    """Vertices with a normal (within 25 degrees of +y), tangent (within 40 degrees of +x) and TexC of their own: attributes that
    really vary across a clipped primitive, and an interpolated tangent that can never line up with the interpolated normal."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = len(pos)
    v = np.zeros(n, VERTEX_DT)
    v["Pos"] = pos
    v["Normal"] = unit(np.stack([rng.uniform(-0.4, 0.4, n), np.ones(n), rng.uniform(-0.4, 0.4, n)], axis=1) * [1, 1, 0.8])
    v["TangentU"] = unit(np.stack([np.ones(n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)], axis=1))
    v["TexC"] = rng.uniform(-2.0, 2.0, (n, 2))
    return v


def textured_ground(rng):
    """A quad through the near plane with tiling texture coordinates, for the material with mipped textures."""
    q = [from_view(p) for p in ([-6.0, -0.9, -5.0], [-6.0, -0.9, 20.0], [6.0, -0.9, 20.0], [6.0, -0.9, -5.0])]
    v = smooth_vertices([q[0], q[1], q[2], q[0], q[2], q[3]], rng)
    v["TexC"] = v["Pos"][:, [0, 2]] * 0.35
    return v


def clip(W=130, H=70, seed=5):
    """Triangles across the near plane, the far plane, behind the eye, 10^6 NDC units outside with one, two and three vertices out,
    across near plane and band together (up to a heptagon: five fan triangles), wholly outside, back-facing, zero-area and sub-pixel
    ones, and one item whose material has mipped textures.  Four items, one with two instances.
    case["fans"]: for each name in CLIP_FANS a case that draws that triangle alone."""
    rng = np.random.default_rng(seed)
    view, viewproj = camera(W, H)
    tris = clip_triangles(W, H)
    names = list(tris)
    both = lambda p: np.concatenate([np.asarray(p), np.asarray(p)[[0, 2, 1]]])
    groups, third = [], (len(names) + 2) // 3
    for k in range(3):
        part = [both(tris[n]) for n in names[k * third:(k + 1) * third]]
        worlds = [IDENTITY, translation((0.75, 0.25, 1.5))] if k == 1 else [IDENTITY]
        groups.append({"v": smooth_vertices(np.concatenate(part), rng), "inst": make_instances(worlds, [k, 3][:len(worlds)])})
    groups.append({"v": textured_ground(rng), "inst": make_instances([IDENTITY], [4])})
    mats = make_materials(5)
    mats["DiffuseMapIndex"][:4] = 7; mats["NormalMapIndex"][:4] = 7          # outside the texture table: white, flat normal
    mats["DiffuseMapIndex"][4] = 0; mats["NormalMapIndex"][4] = 1
    case = {"name": "clip", "items": pack(groups, rng), "materials": mats, "textures": pattern_textures(), "view": view, "viewproj": viewproj,
            "W": W, "H": H, "shadow_dim": 95}
    case["fans"] = {n: dict(case, items=[(smooth_vertices(both(tris[n]), rng), np.arange(6, dtype=np.uint32), make_instances([IDENTITY], [0]), 0, 0)])
                    for n in CLIP_FANS}
    return finish(case)


# ---- case `mixed` -----------------------------------------------------------------------------------------------------------
def mixed(seed):
    """A random blend under the perspective camera: a random half of the clipping subjects, right triangles and slivers of random
    pixel-box sizes with a view depth of their own per vertex, stacks of exact duplicates spread over items and instances, a small
    triangulated patch, empty items in between; about a dozen items over one vertex and one index buffer."""
    W, H = MIXED_SIZES[seed % len(MIXED_SIZES)]
    rng = np.random.default_rng(100 + seed)
    view, viewproj = camera(W, H)
    P = lambda p, zv: from_ndc(*px_to_ndc(np.asarray(p, np.float64), W, H), zv, W, H)
    both = lambda p: np.concatenate([np.asarray(p), np.asarray(p)[[0, 2, 1]]])
    groups = []
    tris = clip_triangles(W, H)
    names = [n for n in tris if rng.random() < 0.5]
    for part in (names[0::2], names[1::2]):
        if part:
            groups.append({"v": smooth_vertices(np.concatenate([both(tris[n]) for n in part]), rng), "inst": make_instances([IDENTITY], [0])})
    # boxes: right triangles and slivers, each vertex at its own depth
    for _ in range(3):
        tri = []
        for _ in range(int(rng.integers(4, 9))):
            bw, bh = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            ox, oy = int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1))
            shape = [((ox, oy), (ox + bw, oy), (ox, oy + bh)), ((ox, oy), (ox + bw, oy + bh), (max(ox + bw - 1.5, ox), oy + bh))][int(rng.integers(0, 2))]
            tri.append(facing(np.array([shape], np.float64))[0])
        pos = np.array([[P(q, rng.uniform(2.0, 90.0)) for q in t] for t in tri])
        groups.append({"v": flat_triangles(pos, unit(rng.normal(size=(len(pos), 3))), rng),
                       "inst": make_instances([IDENTITY], [int(rng.integers(0, 6))])})
    # stacks: the same triangles in three items, one of them instanced with overlapping copies
    nt = int(rng.integers(3, 7))
    tri = facing(rng.uniform(0.0, 1.0, (nt, 3, 2)) * [W, H])
    pos = np.array([[P(q, 12.0) for q in t] for t in tri])
    for k in range(3):
        worlds = [IDENTITY, translation((0.5, 0.0, 0.0)), translation((0.0, -0.25, 0.0))] if k == 1 else [IDENTITY]
        groups.append({"v": flat_triangles(pos, unit(rng.normal(size=(nt, 3))), rng),
                       "inst": make_instances(worlds, rng.integers(0, 6, len(worlds)))})
    # a triangulated patch at one depth
    m = 5
    gxy = np.stack(np.meshgrid(np.linspace(0.1 * W, 0.9 * W, m), np.linspace(0.1 * H, 0.9 * H, m)), axis=-1) + rng.uniform(-0.08, 0.08, (m, m, 2)) * [W, H]
    tri = []
    for j in range(m - 1):
        for i in range(m - 1):
            a, b, c, d = gxy[j, i], gxy[j, i + 1], gxy[j + 1, i + 1], gxy[j + 1, i]
            tri += [(a, b, c), (a, c, d)]
    pos = np.array([[P(q, 25.0) for q in t] for t in facing(np.array(tri))])
    groups.append({"v": flat_triangles(pos, unit(rng.normal(size=(len(pos), 3))), rng), "inst": make_instances([IDENTITY], [1])})
    groups = [groups[k] for k in rng.permutation(len(groups))]
    for kind in (NO_INDICES, NO_INSTANCES, NO_INDICES):
        groups.insert(int(rng.integers(0, len(groups) + 1)), kind)
    return finish({"name": "mixed-%d" % seed, "items": pack(groups, rng), "materials": make_materials(6), "view": view, "viewproj": viewproj,
                   "W": W, "H": H, "shadow_dim": (96, 61, 34, 95, 33, 64)[seed % 6]})


def all_cases():
    """Every case of the tier, by name (generated on demand)."""
    gens = {"stack": stack, "stack-empties": lambda: stack(leading_empties=True), "grid": grid, "clip": clip}
    gens.update({"threshold-" + v: (lambda v=v: threshold(v)) for v in THRESHOLD})
    gens.update({"mixed-%d" % s: (lambda s=s: mixed(s)) for s in range(6)})
    return gens


_CACHE = {}


def get(name):
    if name not in _CACHE:
        _CACHE[name] = all_cases()[name]()
    return _CACHE[name]


CASE_NAMES = tuple(all_cases())
