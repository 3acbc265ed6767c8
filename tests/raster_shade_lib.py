"""Shading cases for the producer passes: where raster_soup_lib aims at the fixed-function half of the rasteriser,
these cases aim at its shader half -- vertex_shader() (World with a real 3 x 3, TexTransform and MatTransform that are neither
identity nor commuting), the attribute interpolation, the sampler of resolve_pixel() on chains that are not square powers of two, and
the tangent frame on saturated normal maps and degenerate tangents.  Deterministic by seed, numpy only.

A case is the dict raster_soup_lib.finish() produces (items as 5-tuples, materials, textures, view, viewproj, W, H, shadow_dim), so the
runners of the soup tests take it unchanged.  Frames are 130 x 70 or 97 x 61, shadow targets at most 64 x 64.

Matrices are written in the row-vector convention of the shaders (v' = v . M, translation in the last row, as XMMatrixRotationY and
XMMatrixTranslation build them) and stored transposed, as the instance, material and pass records hold them: record()."""
import numpy as np

from oracle_lib import INSTANCE_DT, MATERIAL_DT, VERTEX_DT
import raster_soup_lib as soup
from raster_soup_lib import IDENTITY, camera, from_view, pack, unit

MAX_FRAME_PIXELS, MAX_SHADOW_DIM, MAX_TRIANGLES = 130 * 70, 64, 600


# ---- matrices -------------------------------------------------------------------------------------------------------
def record(m4):
    """A row-vector-convention 4 x 4 as the 16 floats a record stores: transposed."""
    return np.ascontiguousarray(np.asarray(m4, np.float64).T, np.float32).reshape(16)


def affine(m3=None, t=(0.0, 0.0, 0.0)):
    m = np.eye(4)
    if m3 is not None:
        m[:3, :3] = m3
    m[3, :3] = t
    return m


def rotation(axis, angle):
    """Rotation by `angle` about `axis` for row vectors (the transpose of Rodrigues' matrix for column vectors)."""
    x, y, z = unit(axis)
    c, s = np.cos(angle), np.sin(angle)
    k = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return (c * np.eye(3) + s * k + (1.0 - c) * np.outer([x, y, z], [x, y, z])).T


# XMMatrixRotationX / Y / Z by +-90 degrees: signed permutation matrices, exact in every format
QUARTER_TURNS = {
    "x+": [[1, 0, 0], [0, 0, 1], [0, -1, 0]], "x-": [[1, 0, 0], [0, 0, -1], [0, 1, 0]],
    "y+": [[0, 0, -1], [0, 1, 0], [1, 0, 0]], "y-": [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
    "z+": [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], "z-": [[0, -1, 0], [1, 0, 0], [0, 0, 1]],
}


def uv_matrix(m2=((1.0, 0.0), (0.0, 1.0)), t=(0.0, 0.0)):
    """A texture transform that acts in the uv plane only: (u, v, 0, 1) . M = (u, v) . m2 + t."""
    m = np.eye(4)
    m[:2, :2] = m2
    m[3, :2] = t
    return m


def uv_rotation(a):
    return np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])


def rolled_camera(W, H):
    """(View, ViewProj) of soup.camera() turned by 0.4 rad about a skew axis of view space (mostly roll, some yaw and pitch): all
    nine entries of View's 3 x 3 are non-zero and pairwise different."""
    view, viewproj = camera(W, H)
    V, VP = view.reshape(4, 4).T.astype(np.float64), viewproj.reshape(4, 4).T.astype(np.float64)
    P = np.linalg.inv(V) @ VP
    V2 = V @ affine(rotation((0.3, -0.5, 1.0), 0.4))
    v = record(V2)
    m3 = v.reshape(4, 4)[:3, :3].reshape(-1)
    assert (m3 != 0).all() and len(np.unique(m3)) == 9
    return v, record(V2 @ P)


def make_instances(worlds, tex_transforms, material_indices):
    inst = np.zeros(len(worlds), INSTANCE_DT)
    inst["World"] = [record(w) for w in worlds]
    inst["TexTransform"] = [record(t) for t in tex_transforms]
    inst["MaterialIndex"] = material_indices
    return inst


def make_materials(n, dmap, nmap, mat_transforms=None):
    """n materials, each with its own albedo, roughness and metalness (never 0.5, the default of a material outside the buffer)."""
    m = np.zeros(n, MATERIAL_DT)
    k = np.arange(n)
    m["DiffuseAlbedo"] = np.stack([0.5 + (k % 4) / 8.0, 1.0 - (k % 3) / 8.0, 0.625 + (k % 2) / 4.0, np.ones(n)], axis=1)
    m["FresnelR0"] = 0.1
    m["Roughness"] = 0.0625 + k / 32.0
    m["Metalness"] = 0.96875 - k / 32.0
    assert not (m["Roughness"] == 0.5).any() and not (m["Metalness"] == 0.5).any() and len(np.unique(m["Roughness"])) == n
    m["MatTransform"] = IDENTITY if mat_transforms is None else [record(t) for t in mat_transforms]
    m["DiffuseMapIndex"] = dmap
    m["NormalMapIndex"] = nmap
    return m


def quad(corners, texc, normal, tangent):
    """Two clockwise triangles (0 1 2, 0 2 3) over four corners given clockwise as the camera sees them."""
    v = np.zeros(6, VERTEX_DT)
    k = [0, 1, 2, 0, 2, 3]
    v["Pos"] = np.asarray(corners, np.float64)[k]
    v["TexC"] = np.asarray(texc, np.float64)[k]
    v["Normal"] = np.broadcast_to(np.asarray(normal, np.float64), (4, 3))[k] if np.ndim(normal) == 1 else np.asarray(normal)[k]
    v["TangentU"] = np.broadcast_to(np.asarray(tangent, np.float64), (4, 3))[k] if np.ndim(tangent) == 1 else np.asarray(tangent)[k]
    return v


def view_quad(cx, cy, z, hw, hh, tilt=0.0):
    """Corners (clockwise on screen, top-left first) of a quad centred at view-space (cx, cy, z), turned by `tilt` about its
    horizontal axis (the top edge moves away from the camera), as world positions under soup.camera()."""
    c, s = np.cos(tilt), np.sin(tilt)
    return [from_view([cx + x, cy + y * c, z + y * s]) for x, y in ((-hw, hh), (hw, hh), (hw, -hh), (-hw, -hh))]


def finish(case):
    W, H = case["W"], case["H"]
    assert W * H <= MAX_FRAME_PIXELS and case["shadow_dim"] <= MAX_SHADOW_DIM and soup.input_triangles(case["items"]) <= MAX_TRIANGLES
    case.setdefault("textures", None)
    for k in ("view", "viewproj"):
        case[k] = np.ascontiguousarray(case[k], np.float32).reshape(16)
    return case


# ---- textures -------------------------------------------------------------------------------------------------------
def box_mips(level0):
    from crychic_renderer_amd.geometry import box_mips as bm
    return bm(level0)


def noise_chain(w, h, rng, levels=None, smooth=False):
    """An RGBA8 noise texture w x h with its chain down to 1 x 1 (or cut to `levels`).  smooth: neighbouring texels, also across the
    wrap, differ by at most 2 of 255 in level 0, and every level is a filtered copy: a probe or a level more moves a sample little."""
    if smooth:
        y, x = np.mgrid[0:h, 0:w]
        ph = rng.uniform(0.0, 2.0 * np.pi, (4, 2))
        ax, ay = (min(1.9 * n / (2.0 * np.pi), 60.0) if n > 1 else 0.0 for n in (w, h))      # one texel on: at most 1.9 before rounding
        t = np.stack([128.0 + ax * np.sin(2.0 * np.pi * x / w + ph[c, 0]) + ay * np.cos(2.0 * np.pi * y / h + ph[c, 1]) for c in range(4)], axis=-1)
        t = np.round(t).astype(np.uint8)
    else:
        t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    chain = box_mips(t)
    return chain[:levels] if levels else chain


def grey_levels(chain):
    """The chain with level k replaced by the solid grey 20 (k + 1): a sample then names the level of detail it was taken at."""
    return [np.full_like(lv, 20 * (k + 1)) for k, lv in enumerate(chain)]


def coordinate_texture(size=32):
    """Texel (x, y) holds (8 x, 8 y, 77, 255): a sample decodes to the texel coordinates it was taken at.  Mipped."""
    y, x = np.mgrid[0:size, 0:size]
    t = np.zeros((size, size, 4), np.uint8)
    t[..., 0] = 8 * x; t[..., 1] = 8 * y; t[..., 2] = 77; t[..., 3] = 255
    return box_mips(t)


def saturated_normal_map():
    """12 x 10 texels in 2 x 2 blocks, each block one of the 27 combinations of 0, 128 and 255 in r, g, b (three repeat)."""
    t = np.zeros((10, 12, 4), np.uint8)
    vals = (0, 128, 255)
    for b in range(30):
        k = b % 27
        bx, by = b % 6, b // 6
        t[2 * by:2 * by + 2, 2 * bx:2 * bx + 2, :3] = (vals[k % 3], vals[(k // 3) % 3], vals[k // 9])
    t[..., 3] = 255
    return t


# ---- case `world` ---------------------------------------------------------------------------------------------------
def dome(rng, n=3):
    """A shallow paraboloid cap over [-1.3, 1.3] x [-0.9, 0.9], apex towards -z, as unshared triangle vertices: the front sheet
    (clockwise seen from -z, normals towards -z) and the back sheet (the same triangles wound the other way, normals negated).
    Normals and tangents are per vertex and not of unit length (0.5 ... 2); the tangent leans out of the tangent plane.
    Returns (front, back)."""
    g = np.linspace(-1.0, 1.0, n + 1)
    u, v = np.meshgrid(g, g)                                  # v: rows
    pos = np.stack([1.3 * u, 0.9 * v, 0.3 * (u * u + v * v) - 0.3], axis=-1)
    du = np.stack([np.full_like(u, 1.3), np.zeros_like(u), 0.6 * u], axis=-1)
    dv = np.stack([np.zeros_like(u), np.full_like(u, 0.9), 0.6 * v], axis=-1)
    nrm = unit(np.cross(dv, du))                              # towards -z
    assert (nrm[..., 2] < 0).all()
    nrm = nrm * rng.uniform(0.5, 2.0, u.shape + (1,))
    tan = (unit(du) + 0.3 * unit(nrm)) * rng.uniform(0.5, 2.0, u.shape + (1,))
    tex = np.stack([u + 1.0, 1.0 - v], axis=-1)               # [0, 2]^2, v down
    tri = []
    for j in range(n):
        for i in range(n):
            p00, p10, p01, p11 = (j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1)
            tri += [(p00, p01, p11), (p00, p11, p10)]         # up, then right: clockwise seen from -z with y up
    idx = np.array(tri).reshape(-1, 2)

    def sheet(order, sign):
        k = idx.reshape(-1, 3, 2)[:, order].reshape(-1, 2)
        out = np.zeros(len(k), VERTEX_DT)
        out["Pos"] = pos[k[:, 0], k[:, 1]]; out["Normal"] = sign * nrm[k[:, 0], k[:, 1]]
        out["TangentU"] = tan[k[:, 0], k[:, 1]]; out["TexC"] = tex[k[:, 0], k[:, 1]]
        return out
    return sheet([0, 1, 2], 1.0), sheet([0, 2, 1], -1.0)


WORLD_TWIN = rotation((1.0, 0.4, 0.2), 0.35) * np.array([[1.1], [0.9], [1.2]])        # diag(s) . R: scale first, then the rotation
WORLD_MATRICES = (
    [(k, np.array(m, np.float64)) for k, m in QUARTER_TURNS.items()] +
    [("skew", rotation((1.0, 2.0, -0.5), 1.1)),
     ("rot-scale", np.diag([1.3, 0.6, 0.9]) @ rotation((0.2, 1.0, 0.3), 0.7)),
     ("shear", np.array([[1.0, 0.45, 0.2], [-0.3, 1.0, 0.35], [0.25, -0.4, 1.0]])),
     ("twin", WORLD_TWIN),
     ("mirror", np.diag([-1.0, 1.0, 1.0]) @ WORLD_TWIN),
     ("small", 0.7 * rotation((-1.0, 0.3, 0.8), 2.0))])
WORLD_SPOTS = [(x, y) for y in (1.6, 0.0, -1.6) for x in (-3.6, -1.2, 1.2, 3.6)]


def world(seed=21):
    """Twelve instances of a two-sided dome (36 triangles each: the lanes of one setup workgroup straddle instances), each under its
    own World -- the six exact quarter turns, a rotation about a skew axis, rotation x non-uniform scale, a shear, a mirror and its
    unmirrored twin, a shrunk rotation -- its own TexTransform and its own material, seen by a camera whose View has nine different
    non-zero entries in its 3 x 3.  Materials alternate between the mipped pattern textures and none.
    case["probes"]: {(instance name, sheet): a case that draws that sheet of that instance alone}, for "twin" and "mirror"."""
    W, H = 130, 70
    rng = np.random.default_rng(seed)
    view, viewproj = rolled_camera(W, H)
    front, back = dome(rng)
    order = [8, 1, 9, 3, 0, 10, 5, 7, 2, 4, 6, 11]             # twin (9) and mirror (10) near the centre of the frame
    names = [WORLD_MATRICES[k][0] for k in order]
    worlds = [affine(WORLD_MATRICES[k][1], from_view([x, y, 6.0 + 0.37 * i])) for i, (k, (x, y)) in enumerate(zip(order, WORLD_SPOTS))]
    assert np.linalg.det(worlds[names.index("mirror")][:3, :3]) < 0 < np.linalg.det(worlds[names.index("twin")][:3, :3])
    n = len(worlds)
    texs = [uv_matrix(uv_rotation(0.2 * i) * (1.0 + 0.25 * i), (0.1 * i, -0.07 * i)) for i in range(n)]
    inst = make_instances(worlds, texs, np.arange(n))
    k = np.arange(n)
    mats = make_materials(n, np.where(k % 2 == 0, 0, 7), np.where(k % 2 == 0, 1, 7))
    assert len(inst) * (len(front) + len(back)) // 3 > 128
    case = {"name": "world", "items": pack([{"v": np.concatenate([front, back]), "inst": inst}], rng), "materials": mats,
            "textures": soup.pattern_textures(), "view": view, "viewproj": viewproj, "W": W, "H": H, "shadow_dim": 64,
            "instances": names}
    case["probes"] = {(nm, sh): dict(case, name="world-%s-%s" % (nm, sh),
                                     items=[(v, np.arange(len(v), dtype=np.uint32), inst[names.index(nm):names.index(nm) + 1], 0, 0)])
                      for nm in ("twin", "mirror") for sh, v in (("front", front), ("back", back))}
    return finish(case)


# ---- case `texc` ----------------------------------------------------------------------------------------------------
Z_W_COLUMNS = np.array([[0.0, 0.0, 0.7, -0.4], [0.0, 0.0, -1.3, 0.6], [0.0, 0.0, 0.9, 0.2], [0.0, 0.0, 0.5, 0.35]])
TEXC_OUTSIDE_MATERIAL = 99


def texc_transforms():
    """(TexTransform, MatTransform or None) per instance.  Where the instance scales the material translates and the reverse, so
    the two never commute.  The z and w columns of a matrix reach TexC only through a later multiplication (GeometryPass.hlsl:39-40
    multiplies the whole float4 by MatTransform), so they sit where nothing follows: in a MatTransform, and in the TexTransform of
    the instance whose material index lies outside the buffer (TexTransform alone applies there)."""
    rst = uv_matrix(uv_rotation(0.6) @ np.diag([2.0, 1.5]), (0.0, 0.0)) @ uv_matrix(t=(0.1, 0.2))
    return [
        (uv_matrix(np.diag([8.0, 8.0])), uv_matrix(t=(0.3, 0.1))),                 # the reference's three scalings
        (uv_matrix(np.diag([1.0, 0.5])), uv_matrix(t=(0.5, 0.25))),
        (uv_matrix(np.diag([1.5, 2.0])), uv_matrix(t=(-0.2, 0.7))),
        (uv_matrix(t=(0.25, 0.5)), uv_matrix(np.diag([2.0, 3.0]))),                # a pure translation
        (rst, uv_matrix(np.diag([0.5, 1.25]), (0.3, 0.0))),                        # rotation . scale . translation
        (uv_matrix(np.diag([1.5, 1.0]), (0.2, 0.3)), uv_matrix(uv_rotation(-0.3), (0.1, 0.4)) + Z_W_COLUMNS - np.diag([0, 0, 1, 1])),
        (uv_matrix(uv_rotation(0.25) * 1.75, (0.4, -0.2)) + Z_W_COLUMNS - np.diag([0, 0, 1, 1]), None),
        (np.eye(4), np.eye(4)),
    ]


def texc(seed=22):
    """Eight instances of one quad, each tilted and at its own place, drawn with a mipped 32 x 32 texture whose texel encodes its own
    coordinates (index 0) and the gentle normal map of the soups (index 1).  texc_transforms() lists what each instance and its
    material apply to TexC; instance 6 names material 99 of 7."""
    W, H = 97, 61
    rng = np.random.default_rng(seed)
    view, viewproj = rolled_camera(W, H)
    v = quad([(-1, 1, 0), (1, 1, 0), (1, -1, 0), (-1, -1, 0)], [(0, 0), (1, 0), (1, 1), (0, 1)], (0.0, 0.0, -1.0), (1.0, 0.0, 0.0))
    tm = texc_transforms()
    spots = [(x, y) for y in (1.35, -1.35) for x in (-3.3, -1.1, 1.1, 3.3)]
    worlds = [affine(rotation((1.0, 0.3 * (i % 3 - 1), 0.1), 0.5 + 0.1 * i) * 1.05, from_view([x, y, 7.0])) for i, (x, y) in enumerate(spots)]
    midx, mts = [], []
    for t, m in tm:
        midx.append(TEXC_OUTSIDE_MATERIAL if m is None else len(mts))
        if m is not None:
            mts.append(m)
    inst = make_instances(worlds, [t for t, _ in tm], midx)
    mats = make_materials(len(mts), 0, 1, mts)
    mats["DiffuseAlbedo"][:, :3] = 1.0                             # G1 is the texture sample itself
    tex = [coordinate_texture(), soup.pattern_textures()[1]]
    return finish({"name": "texc", "items": pack([{"v": v, "inst": inst}], rng), "materials": mats, "textures": tex, "view": view,
                   "viewproj": viewproj, "W": W, "H": H, "shadow_dim": 61})


# ---- case `sampler` -------------------------------------------------------------------------------------------------
# (width, height, stored levels or None for the whole chain); then a single-level texture, a null entry; index 9 is outside
SAMPLER_CHAINS = ((24, 10, None), (5, 3, None), (1, 16, None), (16, 1, None), (64, 64, 3))
SAMPLER_PLAIN, SAMPLER_NULL, SAMPLER_OUTSIDE = 5, 6, 9
# (DiffuseMapIndex, NormalMapIndex): diffuse mipped with a plain normal map, the reverse, both mipped with different sizes, ...
SAMPLER_MATERIALS = ((0, 5), (5, 1), (2, 3), (4, 0), (3, 6), (9, 4), (1, 2))
# TexC per world unit of the ground strip of each material: the strip's pixels run from magnified to beyond the last level
SAMPLER_GROUND_SCALE = (1.2, 3.0, 2.0, 0.5, 5.0, 0.5, 6.0)


def sampler_textures(rng, smooth=False):
    tex = [noise_chain(w, h, rng, lv, smooth) for w, h, lv in SAMPLER_CHAINS]
    tex.append(noise_chain(7, 5, rng, smooth=smooth)[0])          # one array: mipLevels 1
    tex.append(None)
    assert len(tex) == 7 and SAMPLER_OUTSIDE >= len(tex)
    return tex


def sampler(seed=23, smooth=False):
    """Seven ground strips through the near plane, one per material (strong anisotropy; every probe count; every level of every
    chain), under eight quads: constant TexC, TexC along screen x only and along screen y only (a zero minor axis: eight probes),
    TexC in [-3, 3], at exact integers, around +4096 and around -4096, and a tilted one.  The texture table holds chains of
    24 x 10, 5 x 3, 1 x 16 and 16 x 1 down to 1 x 1, a 64 x 64 chain cut to three levels, a single-level 7 x 5 texture and a null
    entry; index 9 lies outside it.  smooth: the same geometry with smooth textures (noise_chain)."""
    W, H = 130, 70
    rng = np.random.default_rng(seed)
    view, viewproj = camera(W, H)
    up, tx = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)
    groups = []
    f = np.linspace(-0.75, 0.75, len(SAMPLER_MATERIALS) + 1) * soup.TAN_HALF_FOV * W / H
    z0, z1 = 0.2, 25.0
    for m, s in enumerate(SAMPLER_GROUND_SCALE):
        c = [from_view([f[m] * z1, -0.9, z1]), from_view([f[m + 1] * z1, -0.9, z1]), from_view([f[m + 1] * z0, -0.9, z0]), from_view([f[m] * z0, -0.9, z0])]
        v = quad(c, [(p[0] * s, p[2] * s) for p in c], unit((0.1, 1.0, -0.05)), unit((1.0, 0.05, 0.2)))
        groups.append({"v": v, "inst": make_instances([np.eye(4)], [np.eye(4)], [m])})
    towards = (0.0, 0.0, -1.0)
    spots = [(x, y) for y in (3.1, 1.05) for x in (-5.7, -1.9, 1.9, 5.7)]
    hw, hh = 1.75, 0.95
    big = 4096.0
    texcs = [
        ([(0.3, 0.7)] * 4, 0.0, 2),                                                  # constant
        ([(-1.5, 0.25), (2.5, 0.25), (2.5, 0.25), (-1.5, 0.25)], 0.0, 2),            # along screen x only
        ([(0.625, -2.0), (0.625, -2.0), (0.625, 1.0), (0.625, 1.0)], 0.0, 3),        # along screen y only
        ([(-3.0, -3.0), (3.0, -2.0), (2.0, 3.0), (-3.0, 2.5)], 1.0, 0),              # [-3, 3]
        ([(-2.0, -1.0), (2.0, -1.0), (2.0, 1.0), (-2.0, 1.0)], 0.0, 6),              # exact integers at the corners and in between
        ([(big - 0.5, big - 0.25), (big + 0.5, big - 0.25), (big + 0.5, big + 0.25), (big - 0.5, big + 0.25)], 1.1, 3),
        ([(-big - 0.5, -big - 0.25), (-big + 0.5, -big - 0.25), (-big + 0.5, -big + 0.25), (-big - 0.5, -big + 0.25)], 1.1, 0),
        ([(0.0, 0.0), (3.0, 0.5), (3.5, 2.0), (-0.5, 1.5)], 1.2, 6),
    ]
    for (x, y), (t, tilt, m) in zip(spots, texcs):
        groups.append({"v": quad(view_quad(x, y, 10.0, hw, hh, tilt), t, towards, tx), "inst": make_instances([np.eye(4)], [np.eye(4)], [m])})
    mats = make_materials(len(SAMPLER_MATERIALS), [d for d, _ in SAMPLER_MATERIALS], [n for _, n in SAMPLER_MATERIALS])
    mats["DiffuseAlbedo"][:, :3] = 1.0
    return finish({"name": "sampler-smooth" if smooth else "sampler", "items": pack(groups, rng), "materials": mats,
                   "textures": sampler_textures(rng, smooth), "view": view, "viewproj": viewproj, "W": W, "H": H, "shadow_dim": 64,
                   "ground_scale": SAMPLER_GROUND_SCALE})


def with_grey_levels(case, swap=False):
    """`sampler` with every chain turned into grey_levels(); swap: with the two map indices of every material exchanged, so the
    chains that serve as normal maps show in G1 too."""
    out = dict(case, name=case["name"] + ("-grey-swapped" if swap else "-grey"))
    out["textures"] = [grey_levels(t) if isinstance(t, list) else t for t in case["textures"]]
    if swap:
        m = case["materials"].copy()
        m["DiffuseMapIndex"], m["NormalMapIndex"] = case["materials"]["NormalMapIndex"], case["materials"]["DiffuseMapIndex"]
        out["materials"] = m
    return out


# ---- case `tbn` -----------------------------------------------------------------------------------------------------
def tbn(seed=24):
    """Six quads under a normal map of saturated texels (0, 128 and 255 per channel in 2 x 2 blocks: normalT components -1,
    1/255 and 1), single-level and mipped: vertex tangents parallel to the normal, zero tangents, normals of length 1e-3 and 1e3,
    and two ordinary ones for contrast.
    Zero and parallel tangents: T = normalize(tangentW - dot(tangentW, N) N) meets DESIGN section 3's `normalize`: the length is
    sqrt(clamp(dot, 2^-100, 2^100)), so a zero vector has "no direction" and normalises to the zero vector (0 * 2^50), not to NaN;
    B = N x 0 = 0 and the bumped normal is normalT.z * N.  A parallel tangent leaves the rounding residue of the subtraction, which
    is either zero or gets a direction of its own; both are finite.  So every plane of this case is finite and the case stays in
    the finite set."""
    W, H = 97, 61
    rng = np.random.default_rng(seed)
    view, viewproj = camera(W, H)
    nrm = unit((0.2, 0.1, -1.0))
    tan = unit(np.cross((0.0, 1.0, 0.0), nrm))
    subjects = [(nrm, nrm * 1.5), (nrm, (0.0, 0.0, 0.0)), (nrm * 1e-3, tan), (nrm * 1e3, tan * 0.5), (nrm, tan), (nrm * 2.0, tan + 0.5 * nrm)]
    spots = [(x, y) for y in (1.8, -1.1) for x in (-4.3, 0.0, 4.3)]
    groups = []
    for i, ((x, y), (n, t)) in enumerate(zip(spots, subjects)):
        v = quad(view_quad(x, y, 9.0, 2.0, 1.3, 0.3 * (i % 2)), [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], n, t)
        jitter = rng.uniform(0.9, 1.1, (6, 1))
        v["Normal"] = v["Normal"] * jitter                      # per-vertex lengths differ a little: the interpolation matters
        groups.append({"v": v, "inst": make_instances([np.eye(4)], [uv_matrix(np.diag([1.0 + i % 2, 1.0]))], [i % 2])})
    sat = saturated_normal_map()
    mats = make_materials(2, [2, 2], [0, 1])
    tex = [sat, box_mips(sat), soup.pattern_textures()[0]]
    return finish({"name": "tbn", "items": pack(groups, rng), "materials": mats, "textures": tex, "view": view, "viewproj": viewproj,
                   "W": W, "H": H, "shadow_dim": 61})


# ---- case `nonfinite` -----------------------------------------------------------------------------------------------
def nonfinite(seed=25):
    """Three items, each a quad one of whose vertices carries a NaN, a +inf or a -inf TexC (so every pixel of its first triangle
    interpolates a non-finite coordinate), over the sampler case's texture table with both maps mipped.  Non-finite coordinates are
    defined to address only out-of-range texels: texel_index sends them to -2 and WRAP brings that back into the
    level, so every plane stays finite."""
    W, H = 97, 61
    rng = np.random.default_rng(seed)
    view, viewproj = camera(W, H)
    groups = []
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        t = np.array([(0.0, 0.0), (2.0, 0.0), (2.0, 1.5), (0.0, 1.5)])
        v = quad(view_quad(-4.0 + 4.0 * i, 0.4 * i, 9.0, 1.9, 2.2, 0.5), t, unit((0.0, 0.3, -1.0)), (1.0, 0.0, 0.0))
        v["TexC"][1] = (bad, 0.5) if i != 1 else (0.25, bad)     # vertex 1 belongs to the first triangle only
        groups.append({"v": v, "inst": make_instances([np.eye(4)], [uv_matrix(np.diag([1.5, 1.0]), (0.1, 0.0))], [(2, 3, 6)[i]])})
    mats = make_materials(len(SAMPLER_MATERIALS), [d for d, _ in SAMPLER_MATERIALS], [n for _, n in SAMPLER_MATERIALS])
    return finish({"name": "nonfinite", "items": pack(groups, rng), "materials": mats, "textures": sampler_textures(rng), "view": view,
                   "viewproj": viewproj, "W": W, "H": H, "shadow_dim": 61})


# ---- the tier -------------------------------------------------------------------------------------------------------
FINITE_CASES = ("world", "texc", "sampler", "tbn")
CASE_NAMES = FINITE_CASES + ("nonfinite",)
_GENS = {"world": world, "texc": texc, "sampler": sampler, "sampler-smooth": lambda: sampler(smooth=True), "tbn": tbn, "nonfinite": nonfinite}
_CACHE = {}


def get(name):
    if name not in _CACHE:
        _CACHE[name] = _GENS[name]()
    return _CACHE[name]
