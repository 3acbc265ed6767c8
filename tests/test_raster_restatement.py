"""The producer passes restated in real arithmetic (numpy float64), the fourth restatement of DESIGN section 3: written from the text of
GeometryPass.hlsl, DrawNormals.hlsl, Shadows.hlsl and NormalSampleToWorldSpace (Common.hlsl:112-128), from D3D's rasterisation rules
(viewport transform, 8-bit sub-pixel snap, integer coverage with the top-left rule, nearest depth, perspective-correct attributes at
the pixel centre, 2 x 2 quad differences as the derivatives) and from the stated definition of the anisotropic sampler
(raster_core.hpp, the comment above sample_texture).  It shares no helper with oracle_lib, the oracle, the kernels or geometry.py, and
is compared with the oracle under a stated tolerance.  It checks transcription -- a swapped matrix index, a dropped translation, a
sampler rule -- and bounds how far the oracle's binary32 evaluation strays from the mathematics; it does not check bits.

Bars.
  G0 - G2: |delta| <= 1e-5 + 1e-4 |ref| (DESIGN section 3's restatement bar), plus, for G1 and G2, 0.98 of the binary32 spacing of
    the pixel's larger texture coordinate.  The second term is a moved bar: on the two quads of `sampler` whose TexC lies around
    +-4096 (spacing 2^-11 and 2^-12: 1 / 85 of a texel of the 24-texel chain) G1 and G2 missed the first term by up to 3.3 and 9.5
    times, on 78 and 229 pixels, all of them at |TexC| >= 4095.75; everywhere else the largest difference is 0.21 of the first
    term.  The binary32 variant of the restatement (restate(binary32=True): TexC rounded where the pixel stage holds it) brings G2
    back to 0.03 of the first term and G1 to one pixel at 1.43, so the differences are binary32's resolution of the coordinate,
    not a transcription's.  Measured in that unit the largest excess is 0.245 spacings; the bar is four times that.  At |TexC| < 8
    the term is below 5e-7.
  The half4 normal of mode 1: |delta| <= 2^-10 |ref| + 2^-24: one half ulp pair of binary16 (the oracle's binary32 value may round
    across one boundary of the 11-bit significand; 2^-24 is the smallest subnormal).
  Depth: +-12 LSB of D24, a moved bar as well.  The oracle interpolates z in double, so what separates it from the mathematics are
    the binary32 roundings behind each vertex's z: z lies in [0.5, 1), where one ulp of binary32 is one LSB of D24, and the last
    three roundings alone (posH.z, 1 / w, their product) come to 1.5 LSB; the roundings further up (posW, the first mads of both
    products, whose partial sums reach the camera's distance from the origin, 15, where the result is 6) add to that, so +-2 LSB
    does not follow and did not hold: 3 LSB on one pixel of `world`, 2 LSB on 1 - 4 % of the pixels, 1 LSB on 16 - 42 %.  With the
    position chain, the clipper and the viewport transform evaluated in binary32 as DESIGN section 3 defines mul(float4, float4x4)
    the restatement's D24 equals the oracle's on every pixel of all three cases, so the differences are those roundings; the bar is
    four times the largest.

Exclusions: only where the restatement itself finds a decision on the edge -- the pixel centre within 2/256 pixel of an edge of the
winning triangle, |major| / |minor| within 1e-3 of an integer (below the cap of 8), the level of detail within 1e-3 of an integer in
[0, levels - 1]; a lookup without any footprint (constant TexC) has no such decision -- and at most 2 % of a case's covered pixels.
The cases must not leave the winner of a pixel to a near tie: the two nearest surfaces of every pixel are at least 8 LSB apart.

Measured: see test_restatement_matches_oracle's docstring."""
import numpy as np
import pytest

import raster_shade_lib as shade

CASES = ("world", "texc", "sampler-smooth")
D24_MAX = 16777215.0
DEPTH_LSB = 12                  # 4 x the largest difference measured (3 LSB), shown to be the vertex stage's binary32 roundings
TEXC_SPACINGS = 0.98            # 4 x the largest excess measured (0.245 spacings of TexC), shown to be binary32's resolution of TexC


# ---- the restatement --------------------------------------------------------------------------------------------------------
def row_matrix(stored):
    """The 16 stored floats as the matrix M of v' = v . M: the records hold M transposed."""
    return np.asarray(stored, np.float64).reshape(4, 4).T


def mul32(v, m):
    """mul(float4, float4x4) as DESIGN section 3 defines its binary32 evaluation: the x product first, then one mad per further
    component.  The product of two binary32 numbers is exact in binary64, so each mad rounds once (twice in about 2^-29 of cases)."""
    v, m = np.asarray(v, np.float32), np.asarray(m, np.float32)
    acc = v[:, 0:1] * m[0:1, :]
    for k in (1, 2, 3):
        acc = (v[:, k:k + 1].astype(np.float64) * m[k:k + 1, :].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def shade_vertices(v, world, tex_transform, mat_transform, viewproj, binary32=False):
    """VS of GeometryPass.hlsl:22-42 (DrawNormals.hlsl:38-64 and Shadows.hlsl:21-44 compute subsets of it): per vertex
    PosH (4), PosW (3), NormalW (3), TangentW (3), TexC (2).  mat_transform None: the material index lies outside the buffer, where
    the project reads TexTransform alone."""
    n = len(v)
    pos4 = np.concatenate([v["Pos"].astype(np.float64), np.ones((n, 1))], axis=1)
    pos_w = pos4 @ world                                            # mul(float4(PosL, 1), gWorld)
    pos_h = pos_w @ viewproj                                        # mul(posW, gViewProj)
    nrm_w = v["Normal"].astype(np.float64) @ world[:3, :3]          # mul(NormalL, (float3x3) gWorld)
    tan_w = v["TangentU"].astype(np.float64) @ world[:3, :3]
    t4 = np.concatenate([v["TexC"].astype(np.float64), np.zeros((n, 1)), np.ones((n, 1))], axis=1)
    t4 = t4 @ tex_transform                                         # mul(float4(TexC, 0, 1), gTexTransform)
    if mat_transform is not None:
        t4 = t4 @ mat_transform                                     # mul(texC, MatTransform).xy
    if binary32:        # the position chain rounded as the definition rounds it; the other outputs rounded once
        pos_w = mul32(pos4, world)
        pos_h = mul32(pos_w, viewproj)
        return np.concatenate([pos_h, pos_w[:, :3], nrm_w, tan_w, t4[:, :2]], axis=1).astype(np.float32)
    return np.concatenate([pos_h, pos_w[:, :3], nrm_w, tan_w, t4[:, :2]], axis=1)


def clip_polygon(poly):
    """Depth clip 0 <= z <= w in clip space (Sutherland-Hodgman; attributes are linear in clip space)."""
    for dist in (lambda p: p[2], lambda p: p[3] - p[2]):
        out = []
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            da, db = dist(a), dist(b)
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                out.append(a + (da / (da - db)) * (b - a))
        poly = out
        if len(poly) < 3:
            return []
    return poly


MUTATIONS = ("world transposed", "transforms swapped", "translation dropped")


def primitives(case, mutation=None, binary32=False):
    """Every triangle of the case in draw order (items, then instances, then triangles; DrawIndexedInstanced reads index
    startIndexLocation + k and adds baseVertexLocation), vertex-shaded and depth-clipped into fans: (3, 15) arrays and the material index."""
    viewproj = row_matrix(case["viewproj"])
    mats = case["materials"]
    out = []
    for v, idx, inst, start, base in case["items"]:
        if v is None or idx is None or inst is None:
            continue
        ind = idx[start:].astype(np.int64) + base
        for rec in inst:
            world, tex_t = row_matrix(rec["World"]), row_matrix(rec["TexTransform"])
            mi = int(rec["MaterialIndex"])
            mat_t = row_matrix(mats[mi]["MatTransform"]) if mi < len(mats) else None
            if mutation == "world transposed":
                world = world.copy(); world[:3, :3] = world[:3, :3].T
            elif mutation == "transforms swapped" and mat_t is not None:
                tex_t, mat_t = mat_t, tex_t
            elif mutation == "translation dropped":
                tex_t = tex_t.copy(); tex_t[3, :3] = 0.0
                if mat_t is not None:
                    mat_t = mat_t.copy(); mat_t[3, :3] = 0.0
            else:
                assert mutation is None or mutation == "transforms swapped"
            vs = shade_vertices(v, world, tex_t, mat_t, viewproj, binary32)
            for t in range(len(ind) // 3):
                poly = clip_polygon([vs[k] for k in ind[3 * t:3 * t + 3]])
                for c in range(1, len(poly) - 1):
                    out.append((np.stack([poly[0], poly[c], poly[c + 1]]), mi))
    return out


def orient(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


class Triangle:
    """Viewport transform, snap to 1/256 pixel, signed area (clockwise on the y-down screen is front)."""

    def __init__(self, verts, W, H):
        w = verts[:, 3]
        self.invw = 1.0 / w
        sx = (verts[:, 0] * self.invw + 1.0) * (0.5 * W)
        sy = (1.0 - verts[:, 1] * self.invw) * (0.5 * H)
        assert (np.abs(sx) < 2.0 ** 21).all() and (np.abs(sy) < 2.0 ** 21).all(), "inside the guard band: only the depth planes clip"
        self.X = np.floor(sx * 256.0 + 0.5).astype(np.int64)
        self.Y = np.floor(sy * 256.0 + 0.5).astype(np.int64)
        self.z = (verts[:, 2] * self.invw).astype(np.float64)       # (a binary32 vertex stage computes all of the above in binary32)
        self.invw = self.invw.astype(np.float64)
        self.attr = verts[:, 4:].astype(np.float64)                 # PosW, NormalW, TangentW, TexC
        X, Y = self.X, self.Y
        self.area2 = int(orient(X[0], Y[0], X[1], Y[1], X[2], Y[2]))

    def edges(self, px, py):
        """The three integer edge functions at the centres of pixels (px, py)."""
        cx, cy = np.asarray(px, np.int64) * 256 + 128, np.asarray(py, np.int64) * 256 + 128
        X, Y = self.X, self.Y
        return [orient(X[a], Y[a], X[b], Y[b], cx, cy) for a, b in ((1, 2), (2, 0), (0, 1))]

    def covered(self, px, py):
        inside = np.ones(np.shape(px), bool)
        X, Y = self.X, self.Y
        for e, (a, b) in zip(self.edges(px, py), ((1, 2), (2, 0), (0, 1))):
            top_left = (Y[b] < Y[a]) or (Y[b] == Y[a] and X[b] > X[a])   # a left edge runs upwards, the top edge runs to the right
            inside &= (e > 0) | ((e == 0) & top_left)
        return inside

    def depth(self, px, py):
        e = self.edges(px, py)
        l1, l2 = e[1] / self.area2, e[2] / self.area2
        return self.z[0] + l1 * (self.z[1] - self.z[0]) + l2 * (self.z[2] - self.z[0])   # z / w is affine on the screen

    def attributes(self, px, py):
        """Perspective-correct attributes: barycentrics weighted by 1 / w."""
        e = self.edges(px, py)
        q = np.stack([e[k] / self.area2 * self.invw[k] for k in range(3)], axis=-1)
        return (q @ self.attr) / q.sum(axis=-1, keepdims=True)

    def edge_distance(self, px, py):
        """Distance of the pixel centres from the nearest edge line, in pixels."""
        X, Y = self.X, self.Y
        d = [np.abs(e) / np.hypot(X[b] - X[a], Y[b] - Y[a]) for e, (a, b) in zip(self.edges(px, py), ((1, 2), (2, 0), (0, 1)))]
        return np.min(d, axis=0) / 256.0


def levels_of(t):
    """A texture of the case as a list of float64 level arrays in [0, 1] (UNORM8: u / 255), or None."""
    if t is None:
        return None
    return [np.asarray(lv, np.float64) / 255.0 for lv in (t if isinstance(t, (list, tuple)) else [t])]


def bilinear_wrap(img, u, v):
    """D3D bilinear with WRAP: texel i has its centre at (i + 0.5) / dim."""
    h, w = img.shape[:2]
    tx, ty = u * w - 0.5, v * h - 0.5
    i0, j0 = np.floor(tx), np.floor(ty)
    fx, fy = (tx - i0)[:, None], (ty - j0)[:, None]
    x0, x1 = np.mod(i0, w).astype(np.int64), np.mod(i0 + 1, w).astype(np.int64)
    y0, y1 = np.mod(j0, h).astype(np.int64), np.mod(j0 + 1, h).astype(np.int64)
    top = img[y0, x0] * (1 - fx) + img[y0, x1] * fx
    bot = img[y1, x0] * (1 - fx) + img[y1, x1] * fx
    return top * (1 - fy) + bot * fy


def sample(textures, index, is_normal_map, u, v, ddx, ddy, r32=lambda a: a):
    """Texture2D.Sample(gsamAnisotropicWrap, uv) as the project defines it.  Returns (rgba (n, 4), on_edge (n,)): on_edge marks the
    pixels whose probe count or level of detail sits within 1e-3 of a decision."""
    n = len(u)
    lv = levels_of(textures[index]) if textures is not None and index < len(textures) else None
    if lv is None:
        return np.tile([0.5, 0.5, 1.0, 1.0] if is_normal_map else [1.0, 1.0, 1.0, 1.0], (n, 1)), np.zeros(n, bool)
    if len(lv) <= 1:
        return bilinear_wrap(lv[0], u, v), np.zeros(n, bool)
    th, tw = lv[0].shape[:2]
    px, py = ddx * [tw, th], ddy * [tw, th]                         # the footprint's axes in level-0 texels
    lx, ly = np.hypot(px[:, 0], px[:, 1]), np.hypot(py[:, 0], py[:, 1])
    major_x = lx >= ly
    pmax, pmin = np.where(major_x, lx, ly), np.where(major_x, ly, lx)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(pmax > 0, pmax / pmin, 1.0)                # no footprint at all: one probe
        probes = np.clip(np.ceil(ratio), 1, 8)
        lod_raw = np.where(pmax > 0, np.log2(pmax / probes), -np.inf)
    top = len(lv) - 1
    lod = np.clip(lod_raw, 0, top)
    l0 = np.floor(lod); frac = lod - l0; l1 = np.minimum(l0 + 1, top)
    axis = np.where(major_x[:, None], ddx, ddy)
    acc = np.zeros((n, 4))
    for k in range(8):
        live = k < probes
        s = (k + 0.5) / probes - 0.5
        uu, vv = r32(u + s * axis[:, 0]), r32(v + s * axis[:, 1])   # (r32: a probe's coordinate is a binary32 number again)
        for level, img in enumerate(lv):
            wt = (l0 == level) * (1 - frac) + (l1 == level) * frac
            use = live & (wt > 0)
            if use.any():
                acc[use] += wt[use, None] * bilinear_wrap(img, uu[use], vv[use])
    footprint = pmax > 0                                            # without one every probe and level reads the same place
    with np.errstate(invalid="ignore"):
        near_ratio = footprint & (ratio < 8 + 1e-3) & (np.abs(ratio - np.round(ratio)) < 1e-3)
        near_lod = footprint & (np.abs(lod_raw - np.round(lod_raw)) < 1e-3) & (lod_raw > -1e-3) & (lod_raw < top + 1e-3)
    return acc / probes[:, None], near_ratio | near_lod


def normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def restate(case, mutation=None, binary32=False):
    """Depth (D24), the view-space normal of DrawNormals.hlsl, G0 - G2 of GeometryPass.hlsl, `covered`, `on_edge` (the exclusions)
    and `margin` (D24 steps between the two nearest surfaces of a pixel).
    binary32: the variant that shows which differences are binary32's and not a transcription's -- the vertex stage's position
    chain, the clipper and the viewport transform evaluated in binary32, and TexC rounded to binary32 where the pixel stage holds
    it (at the pixel, at the quad's other pixels, at every probe).  Everything else stays in real arithmetic."""
    W, H = case["W"], case["H"]
    view3 = row_matrix(case["view"])[:3, :3]
    mats, textures = case["materials"], case["textures"]
    tris = []
    r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if binary32 else (lambda a: a)
    for verts, mi in primitives(case, mutation, binary32):
        t = Triangle(verts, W, H)
        if t.area2 > 0:                                             # back faces and zero areas are culled
            t.material = mi
            tris.append(t)
    depth = np.full((H, W), 1 << 24, np.int64); second = depth.copy()
    winner = np.full((H, W), -1, np.int64)
    for k, t in enumerate(tris):
        x0, x1 = max(int(np.ceil((t.X.min() - 128) / 256.0)), 0), min(int(np.floor((t.X.max() - 128) / 256.0)), W - 1)
        y0, y1 = max(int(np.ceil((t.Y.min() - 128) / 256.0)), 0), min(int(np.floor((t.Y.max() - 128) / 256.0)), H - 1)
        if x0 > x1 or y0 > y1:
            continue
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        inside = t.covered(px, py)
        d24 = np.floor(np.clip(t.depth(px, py), 0.0, 1.0) * D24_MAX + 0.5).astype(np.int64)
        box = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        better = inside & (d24 < depth[box])                        # LESS: an equal depth keeps the earlier primitive
        second[box] = np.where(better, depth[box], np.where(inside, np.minimum(second[box], d24), second[box]))
        depth[box] = np.where(better, d24, depth[box])
        winner[box] = np.where(better, k, winner[box])
    covered = winner >= 0
    out = {"depth": np.where(covered, depth, 0xFFFFFF), "covered": covered, "margin": np.where(covered, second - depth, 1 << 24),
           "normal": np.zeros((H, W, 3)), "g0": np.zeros((H, W, 4)), "g1": np.zeros((H, W, 4)), "g2": np.zeros((H, W, 4)),
           "on_edge": np.zeros((H, W), bool), "texc_max": np.zeros((H, W))}
    for k in np.unique(winner[covered]):
        t = tris[k]
        py, px = np.nonzero(winner == k)
        a = t.attributes(px, py)
        pos_w, nrm, tan, uv = a[:, 0:3], normalize(a[:, 3:6]), a[:, 6:9], r32(a[:, 9:11])     # PS: pin.NormalW = normalize(pin.NormalW)
        out["normal"][py, px] = nrm @ view3                         # DrawNormals.hlsl:91
        # ddx, ddy of TexC: differences inside the pixel's 2 x 2 quad, of this triangle's own plane equations
        qx, qy = px & ~1, py & ~1
        ddx = r32(r32(t.attributes(qx + 1, py)[:, 9:11]) - r32(t.attributes(qx, py)[:, 9:11]))
        ddy = r32(r32(t.attributes(px, qy + 1)[:, 9:11]) - r32(t.attributes(px, qy)[:, 9:11]))
        if t.material < len(mats):
            m = mats[t.material]
            albedo, rough, metal = m["DiffuseAlbedo"][:3].astype(np.float64), float(m["Roughness"]), float(m["Metalness"])
            dmap, nmap = int(m["DiffuseMapIndex"]), int(m["NormalMapIndex"])
        else:                                                       # MaterialData's defaults (FrameResource.h:17-27)
            albedo, rough, metal, dmap, nmap = np.ones(3), 0.5, 0.5, 0, 0
        dtex, e1 = sample(textures, dmap, False, uv[:, 0], uv[:, 1], ddx, ddy, r32)
        ntex, e2 = sample(textures, nmap, True, uv[:, 0], uv[:, 1], ddx, ddy, r32)
        # NormalSampleToWorldSpace, Common.hlsl:112-128
        normal_t = 2.0 * ntex[:, :3] - 1.0
        T = normalize(tan - (tan * nrm).sum(-1, keepdims=True) * nrm)
        B = np.cross(nrm, T)
        bumped = normal_t[:, 0:1] * T + normal_t[:, 1:2] * B + normal_t[:, 2:3] * nrm        # mul(normalT, float3x3(T, B, N))
        out["g0"][py, px] = np.concatenate([pos_w, np.full((len(px), 1), metal)], axis=1)    # EncodePBRToGBuffer, GBuffer.hlsl:22-31
        out["g1"][py, px] = np.concatenate([albedo * dtex[:, :3], np.full((len(px), 1), rough)], axis=1)
        out["g2"][py, px] = np.concatenate([bumped, np.ones((len(px), 1))], axis=1)
        out["on_edge"][py, px] = (t.edge_distance(px, py) < 2.0 / 256.0) | e1 | e2
        out["texc_max"][py, px] = np.abs(uv).max(axis=1)
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------
_ORACLE, _RESTATED = {}, {}


def oracle_planes(oracle, case):
    import oracle_lib
    if case["name"] not in _ORACLE:
        run = lambda mode: oracle_lib.rasterize(oracle, mode, case["view"], case["viewproj"], case["items"], case["materials"],
                                                case["textures"], case["W"], case["H"])
        nd, gb = run(1), run(2)
        assert np.array_equal(nd["depth"], gb["depth"])
        _ORACLE[case["name"]] = {"depth": gb["depth"].astype(np.int64), "normal": nd["normal"][..., :3].astype(np.float64),
                                 "g0": gb["g0"].astype(np.float64), "g1": gb["g1"].astype(np.float64), "g2": gb["g2"].astype(np.float64)}
    return _ORACLE[case["name"]]


def restated(name):
    if name not in _RESTATED:
        _RESTATED[name] = restate(shade.get(name))
    return _RESTATED[name]


def compare(mine, ref, texc_spacings=TEXC_SPACINGS):
    """Per plane the largest |delta| / bar over the covered pixels outside the exclusions (<= 1 passes), the excluded share of the
    covered pixels, whether both cover the same pixels, and per plane the number of pixels over the bar."""
    covered = mine["covered"]
    same_cover = np.array_equal(covered, ref["depth"] < 0xFFFFFF)
    keep = covered & (ref["depth"] < 0xFFFFFF) & ~mine["on_edge"]
    spacing = np.spacing(np.maximum(mine["texc_max"], 1e-30).astype(np.float32)).astype(np.float64)[..., None]
    ratio = {"depth": np.abs(mine["depth"] - ref["depth"])[..., None] / DEPTH_LSB,
             "g0": np.abs(mine["g0"] - ref["g0"]) / (1e-5 + 1e-4 * np.abs(ref["g0"])),
             "normal": np.abs(mine["normal"] - ref["normal"]) / (2.0 ** -10 * np.abs(ref["normal"]) + 2.0 ** -24)}
    for k in ("g1", "g2"):
        ratio[k] = np.abs(mine[k] - ref[k]) / (1e-5 + 1e-4 * np.abs(ref[k]) + texc_spacings * spacing)
    worst = {k: float(v.max(-1)[keep].max()) for k, v in ratio.items()}
    over = {k: int((v.max(-1)[keep] > 1.0).sum()) for k, v in ratio.items()}
    return worst, float((covered & mine["on_edge"]).sum() / covered.sum()), same_cover, over


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_oracle(oracle, name):
    """Measured, largest |delta| / bar outside the exclusions (depth: 12 LSB is 1) and the excluded share of the covered pixels:
                        depth    G0      G1      G2      normal   excluded
        world           0.25     0.005   0.040   0.051   0.49     1.08 % of 3250
        texc            0.17     0.003   0.142   0.059   0.34     0.32 % of 1887
        sampler-smooth  0.17     0.037   0.324   0.269   0.16     1.90 % of 5644
    Against the first term of their bar alone G1 and G2 of sampler-smooth reach 3.29 and 9.54 (the quads with TexC around +-4096)."""
    mine, ref = restated(name), oracle_planes(oracle, shade.get(name))
    assert mine["covered"].mean() >= 0.2
    assert mine["margin"][mine["covered"]].min() >= 8, "a near tie decides a pixel: change the inputs"
    worst, excluded, same_cover, _ = compare(mine, ref)
    print("restatement vs oracle, %s: %s; excluded %.4f of %d covered pixels" % (name, {k: round(v, 4) for k, v in worst.items()},
                                                                               excluded, mine["covered"].sum()))
    assert same_cover
    assert excluded <= 0.02, excluded
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("mutation,name,planes", [("world transposed", "world", ("normal", "g2")),
                                                  ("transforms swapped", "texc", ("g1",)),
                                                  ("translation dropped", "texc", ("g1",))])
def test_restatement_bites(oracle, mutation, name, planes):
    """The three mistakes no test could see while World was diagonal and the texture transforms were identity, made on purpose in
    the restatement's own inputs: the comparison must fail on the planes that depend on them, and by a wide margin."""
    ref = oracle_planes(oracle, shade.get(name))
    worst, _, _, _ = compare(restate(shade.get(name), mutation), ref)
    print(mutation, name, {k: round(v, 1) for k, v in worst.items()})
    for k in planes:
        assert worst[k] > 100.0, (k, worst[k])


@pytest.mark.parametrize("name", CASES)
def test_binary32_variant_accounts_for_the_moved_bars(oracle, name):
    """What the two moved bars rest on.  With the vertex stage's position chain, the clipper and the viewport transform in binary32
    the restatement's D24 plane equals the oracle's exactly; with TexC rounded to binary32 where the pixel stage holds it, G1 and G2
    meet the first term of their bar alone (all but one pixel of `sampler-smooth`, at 1.43 in G1)."""
    ref = oracle_planes(oracle, shade.get(name))
    mine = restate(shade.get(name), binary32=True)
    worst, _, same_cover, over = compare(mine, ref, texc_spacings=0.0)
    print("binary32 variant, %s: %s, pixels over: %s" % (name, {k: round(v, 4) for k, v in worst.items()}, over))
    assert same_cover and worst["depth"] == 0.0
    assert over["g0"] == 0 and over["normal"] == 0 and over["g1"] + over["g2"] <= 1 and max(worst["g1"], worst["g2"]) < 2.0
