"""Random (incoherent) input planes and perturbed constants for the fuzz parity tests: nothing here looks like a scene --
the point is to drive every sampler / special-value path (border, clamp, NaN, inf, zero-length vectors, huge shadow
coordinates) through oracle, kernel bodies and the device with the same bits."""
import ctypes as C

import numpy as np


def random_case(seed, built_lib, size=None):
    """size = (W, H): force the frame size (the random draws that follow are the same either way)."""
    from crychic_renderer_amd import scene
    rng = np.random.default_rng(seed)
    W = int(rng.integers(17, 100)) * 2
    H = int(rng.integers(17, 70)) * 2
    if size is not None:
        W, H = size
    sd = int(rng.choice([16, 64, 130]))
    cd = int(rng.choice([2, 8, 33]))
    c = scene.Constants(W, H, shadow_dim=sd)
    # --- planes -------------------------------------------------------------------------------------------------
    depth = rng.integers(0, 1 << 24, size=(H, W), dtype=np.uint32)
    depth[rng.random((H, W)) < 0.25] = 0xFFFFFF                         # uncovered
    depth[rng.random((H, W)) < 0.05] = 0
    if rng.random() < 0.35 and W > 16 and H > 16:
        # a smooth depth field (tilted plane + a little noise) with spikes, holes and sky patches: the SSAO tap culling gets
        # blocks it can cull and blocks a single texel spoils
        yy, xx = np.mgrid[0:H, 0:W]
        lo, hi = sorted(rng.integers(1 << 20, (1 << 24) - 1, 2).tolist())
        ramp = lo + (hi - lo) * ((yy * float(rng.random()) + xx * float(rng.random())) / float(H + W))
        depth = (ramp + rng.integers(-40, 41, size=(H, W))).clip(0, 0xFFFFFE).astype(np.uint32)
        k = int(rng.integers(5, 60))
        depth[rng.integers(0, H, k), rng.integers(0, W, k)] = rng.integers(0, 1 << 24, k).astype(np.uint32)
        for _ in range(int(rng.integers(0, 5))):
            y0, x0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
            depth[y0:y0 + int(rng.integers(1, 9)), x0:x0 + int(rng.integers(1, 9))] = 0xFFFFFF
    depth |= rng.integers(0, 256, size=(H, W), dtype=np.uint32) << 24      # stencil byte must be ignored
    nrm = rng.standard_normal((H, W, 4)).astype(np.float16)
    sel = rng.random((H, W))
    nrm[sel < 0.03] = 0.0
    nrm[(sel >= 0.03) & (sel < 0.04), 0] = np.nan
    nrm[(sel >= 0.04) & (sel < 0.05), 1] = np.inf
    nrm[(sel >= 0.05) & (sel < 0.30)] = np.array([0.0, 0.0, -1.0, 0.0], dtype=np.float16)   # flat patches: blur accepts
    g0 = (rng.standard_normal((H, W, 4)) * 20.0).astype(np.float32); g0[..., 3] = rng.random((H, W))
    if rng.random() < 0.4:
        # coherent world positions (a tilted plane receding from the eye, a little noise): whole wavefronts then fall into one
        # shadow cascade, which is what the wave-uniform cascade path of the lighting kernel needs to run at all
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        far = float(rng.choice([25.0, 60.0, 120.0]))
        eye = np.array(list(c.cam.pos), dtype=np.float32)
        g0[..., 0] = eye[0] + (xx / W - 0.5) * 6.0
        g0[..., 1] = eye[1] - 1.0 + rng.standard_normal((H, W)).astype(np.float32) * 0.05
        g0[..., 2] = eye[2] + 2.0 + (1.0 - yy / H) * far
    g1 = rng.random((H, W, 4)).astype(np.float32)
    g2 = rng.standard_normal((H, W, 4)).astype(np.float32)
    sel = rng.random((H, W))
    g2[sel < 0.02, :3] = 0.0
    g0[(sel >= 0.02) & (sel < 0.03), 0] = np.inf
    g0[(sel >= 0.03) & (sel < 0.04), 1] = np.nan
    g0[(sel >= 0.04) & (sel < 0.05), :3] = 1e30
    g1[(sel >= 0.05) & (sel < 0.06), 3] = 0.0
    g1[(sel >= 0.06) & (sel < 0.07), :3] = -2.0
    g0[(sel >= 0.07) & (sel < 0.08), :3] = np.array(list(c.cam.pos), dtype=np.float32)
    g1[(sel >= 0.08) & (sel < 0.09), 3] = np.nan
    shadow = rng.integers(0, 1 << 24, size=(4, sd, sd), dtype=np.uint32)
    shadow[:, : sd // 2] |= 0x00F00000                                     # mostly-lit half so compares go both ways
    cube = rng.integers(0, 256, size=(6, cd, cd, 4), dtype=np.uint8)
    randvec = rng.integers(0, 256, size=(256, 256, 4), dtype=np.uint8)
    planes = {"depth": depth, "normal": nrm, "g0": g0, "g1": g1, "g2": g2, "shadow": shadow, "cube": cube, "randvec": randvec}
    # --- constants ----------------------------------------------------------------------------------------------
    s, p = c.ssao_cb, c.pass_cb
    s.OcclusionRadius = float(rng.choice([0.05, 0.5, 3.0]))
    s.OcclusionFadeStart = float(rng.choice([0.0, 0.2, 1.0]))
    s.OcclusionFadeEnd = float(rng.choice([1.0, 2.0, s.OcclusionFadeStart]))     # start == end: division by zero
    s.SurfaceEpsilon = float(rng.choice([0.0, 0.05, 0.5]))
    if rng.random() < 0.35:            # a sheared projection: the kernels must leave their sparse-gProjTex fast path
        s.ProjTex[1] = float(rng.choice([0.05, -0.2]))
        s.ProjTex[13] = float(rng.choice([0.0, 0.01]))
    for i in range(3):
        d = rng.standard_normal(3)
        d = d / np.linalg.norm(d) if rng.random() > 0.1 else np.zeros(3)
        p.Lights[i].Direction[:] = [float(x) for x in d]
        p.Lights[i].Strength[:] = [float(x) for x in rng.choice([0.0, 0.1, 1.0, 2.4], size=3)]
    p.AmbientLight[:] = [float(x) for x in rng.random(4)]
    # shadow transforms: keep the cascade matrices but shrink them so random world positions land inside the maps
    for k in range(4):
        for j in range(16):
            p.ShadowTransforms[k][j] = float(p.ShadowTransforms[k][j] * rng.choice([0.2, 1.0]))
    knobs = {
        "blurCount": int(rng.integers(0, 7)), "numDirLights": int(rng.integers(0, 4)),
        "pcfSearchRadius": float(rng.choice([0.0, 2.5 / sd, 10.0 / sd])), "sky": int(rng.integers(0, 2)),
        "ssao_on": bool(rng.random() > 0.15),
    }
    return W, H, planes, c, knobs


def same_floats(a, b):
    """Bit equality, except that any NaN equals any NaN (x86 and gfx950 disagree on the sign / payload of generated NaNs)."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn]))


def sky_probe_case(seed, consts=None, cam=None):
    """Inputs for the SSAO sky-shortcut probe (tests/test_hostsim_parity.py::test_sky_shortcut_is_exact and its device twin): a sky
    field with small patches of geometry within OcclusionFadeEnd of the far distance.
    cam: the camera in place of the reference one; consts: a scene.Constants to use as it is (its W x H is the frame's size).  The
    patches sit at 0.99 .. 0.99999 of the camera's far distance and are encoded with the constants' own A and B."""
    import oracle_lib
    from crychic_renderer_amd import scene
    rng = np.random.default_rng(1000 + seed)
    W, H = int(rng.choice([640, 770, 1024])), int(rng.choice([384, 400, 512]))       # several cells of the coarse geometry map each way
    if consts is not None:
        W, H = consts.W, consts.H
    c = consts if consts is not None else scene.Constants(W, H, shadow_dim=64, cam=cam)
    far = float(c.cam.farZ)
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    A, B = c.ssao_cb.Proj[10], c.ssao_cb.Proj[11]
    depth = np.full((H, W), 0xFFFFFF, dtype=np.uint32)
    # sky normals facing the camera (with the reference's clear value (0, 0, 1) an occluder in front of a far-plane pixel always
    # has dp = 0): random unit-ish vectors or (0, 0, -1), so that a tap landing on a patch really contributes
    normal = np.zeros((H, W, 4), dtype=np.float16); normal[..., 2] = -1.0
    if seed % 2:
        normal[..., :3] = rng.standard_normal((H, W, 3)).astype(np.float16)
    for _ in range(int(rng.integers(1, 5))):
        pw, ph = int(rng.integers(1, 24)), int(rng.integers(1, 16))
        x0, y0 = int(rng.integers(0, W - pw)), int(rng.integers(0, H - ph))
        if seed >= 12:      # hug the corner of a cell of the coarse geometry map (128 x 32 texels, columns offset by -2): worst case for the reach bound
            pw, ph = int(rng.integers(1, 3)), int(rng.integers(1, 3))
            x0 = min(W - pw, 128 * int(rng.integers(1, W // 128)) - 2 - int(rng.integers(0, 2)) * pw)
            y0 = min(H - ph, 32 * int(rng.integers(1, H // 32)) - int(rng.integers(0, 2)) * ph)
        vz = rng.uniform(far * 0.99, far * 99.999 / 100.0, size=(ph, pw))   # inside the occluding band of a pixel at the far distance
        zndc = A + B / vz
        depth[y0:y0 + ph, x0:x0 + pw] = np.clip(np.round(zndc * 16777215.0), 0, 0xFFFFFF).astype(np.uint32)
        normal[y0:y0 + ph, x0:x0 + pw, :3] = rng.standard_normal((ph, pw, 3)).astype(np.float16)
    if seed % 4 == 3:
        normal[rng.random((H, W)) < 0.01, 0] = np.inf                        # a non-finite normal keeps its wavefront off the shortcut
    randvec = rng.integers(0, 256, size=(256, 256, 4), dtype=np.uint8)
    if seed >= 12:
        randvec = (rng.integers(0, 2, size=(256, 256, 4), dtype=np.uint8) * 255).astype(np.uint8)      # |randVec| = sqrt(3): the longest reflected offsets
    return W, H, c, scb, depth, normal, randvec


def clear_cell_probe_case(seed, consts=None, cam=None):
    """Inputs for the clear-cell rule of the SSAO depth pass (ssao_core.hpp "clear cells"): sky next to geometry that hugs the near
    plane, an occlusion radius that puts taps at and behind the camera (q.z < 1e-3: never culled, landing anywhere -- mostly beyond
    the plane's edge, which is clear by definition) and a few non-finite normals (pixels that may not cull at all).
    consts / cam: as sky_probe_case takes them; the geometry sits at 1.0 .. 1.8 times the camera's near distance and the occlusion
    radius is three times that distance."""
    import oracle_lib
    W, H, c, scb, depth, normal, randvec = sky_probe_case(seed, consts, cam)
    rng = np.random.default_rng(77 + seed)
    A, B = c.ssao_cb.Proj[10], c.ssao_cb.Proj[11]
    near = float(c.cam.nearZ)
    x0, x1 = W // 5, W // 5 + 90 + 8 * seed
    vz = rng.uniform(1.0, 1.8, size=(H // 2, x1 - x0)) * near
    depth[H // 4:H // 4 + H // 2, x0:x1] = np.clip(np.round((A + B / vz) * 16777215.0), 0, 0xFFFFFF).astype(np.uint32)
    normal[H // 4:H // 4 + H // 2, x0:x1, :3] = rng.standard_normal((H // 2, x1 - x0, 3)).astype(np.float16)
    normal[rng.random((H, W)) < 0.002, 1] = np.nan
    c.ssao_cb.OcclusionRadius = 3.0 * near
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    return W, H, c, scb, depth, normal, randvec


def rough_wall_case(seed, W, H, sky_blocks, consts=None, cam=None):
    """Frames for the blur chain's tile hand-off (tests/test_blur_chain_handoff.py): a "rough wall" -- view depth uniform in
    [6.0, 6.6] per texel, normals (0.5 n1, 0.5 n2, -1) with n1, n2 standard normal, random randvec.  About 90 % of the texels
    come out occluded, every texel changes under the blur and NO tile settles, so every tile of the chain takes part in the
    hand-off and a stale apron read changes the result.  sky_blocks: rectangles of sky (clear depth, normal (0, 0, -1)) on a grid
    of 256 x 96 full-res texels (2 x 3 blur tiles), each present with probability 1/2 -- tiles inside them settle and their
    workgroups return at once, which makes the load uneven.
    consts / cam: as sky_probe_case takes them (consts must be W x H); a camera whose frustum does not hold [6.0, 6.6] gets the
    wall scaled to the geometric middle of its near and far distances.  Returns (c, scb, depth, normal, randvec)."""
    import oracle_lib
    from crychic_renderer_amd import scene
    rng = np.random.default_rng(seed)
    c = consts if consts is not None else scene.Constants(W, H, shadow_dim=64, cam=cam)
    assert (c.W, c.H) == (W, H)
    A, B = c.ssao_cb.Proj[10], c.ssao_cb.Proj[11]
    near, far = float(c.cam.nearZ), float(c.cam.farZ)
    k = 1.0 if near < 6.0 and far > 6.6 else (near * far) ** 0.5 / 6.3
    vz = rng.uniform(6.0, 6.6, size=(H, W)) * k
    depth = np.clip(np.round((A + B / vz) * 16777215.0), 0, 0xFFFFFE).astype(np.uint32)
    normal = np.zeros((H, W, 4), np.float16); normal[..., 2] = -1.0
    normal[..., :2] = (0.5 * rng.standard_normal((H, W, 2))).astype(np.float16)
    randvec = rng.integers(0, 256, size=(256, 256, 4), dtype=np.uint8)
    if sky_blocks:
        rng = np.random.default_rng(100 + seed)
        for by in range(0, H, 96):
            for bx in range(0, W, 256):
                if rng.random() < 0.5:
                    depth[by:by + 96, bx:bx + 256] = 0xFFFFFF
                    normal[by:by + 96, bx:bx + 256, :3] = (0, 0, -1)
    scb = oracle_lib.as_oracle_cb(c.ssao_cb, oracle_lib.OrSsaoConstants)
    return c, scb, depth, normal, randvec


def cull_probe_case(seed, W=256, H=160, consts=None, cam=None):
    """Frames for the SSAO tap culling (ssao_core.hpp): the reference scene -- open ground, where most taps are culled -- with what
    the nearest-depth bound must not miss: single near texels (spikes a fraction of a block wide), texels just in front of their
    surroundings (around SurfaceEpsilon in view space), holes to the far plane, depth 0, a few small patches, NaN normals, and one
    of several SurfaceEpsilon values.
    consts / cam: as sky_probe_case takes them (consts must be W x H): the scene is then ray-cast through that camera, and depth
    is encoded with its near and far distances.  Returns (W, H, constants, depth, normal, randvec)."""
    import scene_util
    if consts is not None or cam is not None:
        from crychic_renderer_amd import scene
        consts = consts if consts is not None else scene.Constants(W, H, shadow_dim=64, cam=cam)
        assert (consts.W, consts.H) == (W, H)
        pl = scene.make_scene(W, H, shadow_dim=consts.shadow_dim, cube_dim=8, device="cpu", consts=consts)
    else:
        pl = scene_util.cpu_scene(W, H, 64, 8)
    p = scene_util.np_planes(pl)
    c = pl["consts"]
    rng = np.random.default_rng(1234 + seed)
    depth, normal = p["depth"].copy(), p["normal"].copy()
    if seed > 0:
        n = 60
        ys, xs = rng.integers(0, H, n), rng.integers(0, W, n)
        kind = rng.integers(0, 4, n)
        base = depth[ys, xs] & 0xFFFFFF
        spike = np.where(kind == 0, rng.integers(0, 1 << 22, n),
                np.where(kind == 1, base - rng.integers(0, 200, n).clip(max=base),
                np.where(kind == 2, 0xFFFFFF, 0))).astype(np.uint32)
        depth[ys, xs] = spike
        for _ in range(6):
            y0, x0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 4))
            depth[y0:y0 + int(rng.integers(1, 5)), x0:x0 + int(rng.integers(1, 5))] = int(rng.integers(0, 1 << 24))
        normal[rng.integers(0, H, 40), rng.integers(0, W, 40), 0] = np.nan
        c.ssao_cb.SurfaceEpsilon = float([0.05, 0.0, 0.5, 0.05, 1e-4, 0.05][seed % 6])
    return W, H, c, depth, normal, p["randvec"]


# ---- frames for the tiled cull of the local lights (tests/test_light_cull_host.py, tests/test_light_cull_gpu.py) ------------------
LIGHT_DT = np.dtype([("Strength", "<f4", 3), ("FalloffStart", "<f4"), ("Direction", "<f4", 3), ("FalloffEnd", "<f4"),
                     ("Position", "<f4", 3), ("SpotPower", "<f4")])        # crychic_light
CULL_W, CULL_H = 130, 70            # three tile columns (the last 2 pixels wide), a last tile row of 2 rows
CULL_ROW_RANGES = ((0, 36), (36, 22), (58, 12))      # the third is not anchored on a multiple of the tile height
CULL_FALLOFF_END = np.array([0.5, 2.0, 4.0, 10.0, 30.0, 0.0, -1.0, np.nan, np.inf], np.float32)
CULL_FALLOFF_END_P = np.array([0.22, 0.2, 0.15, 0.13, 0.08, 0.05, 0.05, 0.06, 0.06])


def lights_from_records(rec):
    """A ctypes array of the product's Light from a LIGHT_DT record array."""
    from crychic_renderer_amd._lib import Light
    rec = np.ascontiguousarray(rec, LIGHT_DT)
    return (Light * len(rec)).from_buffer_copy(rec.tobytes())


def cull_lights(rng, n, eye, far, regular, infinite_end=True):
    """n local lights: positions half N(0, 20) and half spread along the coherent plane of random_case, FalloffEnd from
    CULL_FALLOFF_END (infinite_end False: 0.5 in the place of +inf, and no infinite position with a NaN FalloffEnd), FalloffStart from {0, 1, FalloffEnd}, SpotPower from {0, 1, 8, 64}, un-normalised directions, about 1 % of
    the positions with a NaN component and 1 % with an infinite one.  The first `regular` lights are finite with FalloffEnd 10 or
    30 and FalloffStart 1 (what the shadow transform builders accept)."""
    L = np.zeros(n, LIGHT_DT)
    pos = (rng.standard_normal((n, 3)) * 20.0).astype(np.float32)
    plane = rng.random(n) < 0.5
    along = np.stack([eye[0] + rng.uniform(-3.0, 3.0, n), eye[1] - 1.0 + rng.standard_normal(n) * 0.5, eye[2] + 2.0 + rng.random(n) * far], 1)
    pos[plane] = along[plane].astype(np.float32)
    L["FalloffEnd"] = rng.choice(CULL_FALLOFF_END, n, p=CULL_FALLOFF_END_P)
    start = rng.integers(0, 3, n)
    L["FalloffStart"] = np.where(start == 0, np.float32(0.0), np.where(start == 1, np.float32(1.0), L["FalloffEnd"]))
    L["Strength"] = rng.choice(np.array([0.0, 0.1, 1.0, 2.4], np.float32), (n, 3))
    L["Direction"] = (rng.standard_normal((n, 3)) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)
    L["SpotPower"] = rng.choice(np.array([0.0, 1.0, 8.0, 64.0], np.float32), n)
    odd = rng.random(n)
    comp = rng.integers(0, 3, n)
    for k in np.nonzero(odd < 0.02)[0]:
        pos[k, comp[k]] = np.nan if odd[k] < 0.01 else (np.inf if odd[k] < 0.015 else -np.inf)
    if not infinite_end:          # no light that is in range everywhere with a NaN term (light_cull_case)
        L["FalloffEnd"][np.isinf(L["FalloffEnd"])] = 0.5
        L["FalloffEnd"][np.isinf(pos).any(1) & np.isnan(L["FalloffEnd"])] = 4.0
    m = min(regular, n)
    pos[:m] = along[:m].astype(np.float32)
    L["FalloffEnd"][:m] = rng.choice(np.array([10.0, 30.0], np.float32), m)
    L["FalloffStart"][:m] = 1.0
    L["Position"] = pos
    return L


def light_cull_case(seed, built_lib, n_points=1024, n_spots=1024):
    """A 130 x 70 frame for the tiled cull: random_case's planes and constants (same seed) with the world positions redrawn -- even
    seeds coherent (random_case's tilted plane), odd seeds incoherent (N(0, 20) per pixel) -- and non-finite positions put in by
    tile of the whole frame's 64 x 4 grid: most tiles none, some exactly one, some a few, some all of their covered positions (and
    one such tile at least per frame); a non-finite position is a NaN in one component, in all three, or +-inf in one.
    A light with FalloffEnd = +inf is in range everywhere with an attenuation of NaN ((inf - d) / (inf - FalloffStart)), and so is
    one at an infinite position whose FalloffEnd is NaN (l / d = inf * 0): either turns the radiance of about half of the frame's
    pixels into NaN -- equal to any NaN, so blind to everything else.  Seeds with seed % 4 in (1, 2) draw such lights (one frame of
    every (2k, 2k + 1) pair); the others keep about 98 % of their pixels finite.
    Returns (planes, constants, knobs, point light records, spot light records)."""
    W, H = CULL_W, CULL_H
    _, _, planes, c, knobs = random_case(seed, built_lib, size=(W, H))
    rng = np.random.default_rng(50000 + seed)
    eye = np.array(list(c.cam.pos), dtype=np.float32)
    far = float(rng.choice([25.0, 60.0, 120.0]))
    g0 = planes["g0"].copy()
    if seed % 2 == 0:
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        g0[..., 0] = eye[0] + (xx / W - 0.5) * 6.0
        g0[..., 1] = eye[1] - 1.0 + rng.standard_normal((H, W)).astype(np.float32) * 0.05
        g0[..., 2] = eye[2] + 2.0 + (1.0 - yy / H) * far
    else:
        g0[..., :3] = (rng.standard_normal((H, W, 3)) * 20.0).astype(np.float32)
    covered = (planes["depth"] & 0xFFFFFF) < 0xFFFFFF

    def spoil(y, x):
        kind = int(rng.integers(0, 6))
        if kind < 3:
            g0[y, x, kind] = np.nan
        elif kind == 3:
            g0[y, x, :3] = np.nan
        else:
            g0[y, x, int(rng.integers(0, 3))] = np.inf if kind == 4 else -np.inf

    tiles = [(ty, tx) for ty in range((H + 3) // 4) for tx in range((W + 63) // 64) if covered[4 * ty:4 * ty + 4, 64 * tx:64 * tx + 64].any()]
    forced = {tiles[int(k)]: mode for k, mode in zip(rng.choice(len(tiles), 3, replace=False), ("all", "one", "one"))}
    for ty, tx in tiles:
        ys, xs = np.nonzero(covered[4 * ty:4 * ty + 4, 64 * tx:64 * tx + 64])
        r = rng.random()
        mode = forced.get((ty, tx)) or ("one" if r < 0.14 else "few" if r < 0.25 else "all" if r < 0.30 else None)
        if mode == "all":
            g0[4 * ty + ys, 64 * tx + xs, int(rng.integers(0, 3))] = np.nan
        elif mode is not None:
            for k in rng.choice(len(ys), min(len(ys), 1 if mode == "one" else int(rng.integers(2, 7))), replace=False):
                spoil(4 * ty + ys[k], 64 * tx + xs[k])
    planes = dict(planes, g0=g0)
    points = cull_lights(rng, n_points, eye, far, 4, seed % 4 in (1, 2))
    spots = cull_lights(rng, n_spots, eye, far, 8, seed % 4 in (1, 2))
    return planes, c, knobs, points, spots
