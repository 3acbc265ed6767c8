"""The frames, light sets, families and checkers of the tiled light cull's tests (TEST INFRASTRUCTURE ONLY), shared by
tests/test_light_cull_host.py and tests/test_light_cull_gpu.py.  A case is one fuzz_util.light_cull_case frame (130 x 70, thinned
non-finite world positions, 1024 point + 1024 spot lights) bound the way one local-light kernel family takes it; `reference` runs
the frozen checker that covers the family on it."""
import numpy as np

import env_sh_lib
import fuzz_util
import gbuffer_f16_lib as gf
import gloss_lib
import local_light_lib
import oracle_lib
import point_shadow_lib
from local_lights_util import FIX_ALL, random_maps, spot_transforms, transposed, with_transforms

MAP_DIM = CUBE_DIM = 16            # the smallest shadow maps the entries take

# what each family binds: the light lists, `maps` shadowed spot lights, `cubes` shadowed point lights, the G-buffer format mix, and
# the cube map's use (chain: the derivative chain; gloss: the chain by roughness; sh: the SH9 ambient term from the tail)
FAMILIES = {
    "points": dict(points=True),                                            # light_points_kernel
    "points_spots": dict(points=True, spots=True),                          # light_spots_kernel
    "spot_shadows": dict(spots=True, maps=3),                               # light_spots_shadowed_kernel, spot lights only
    "point_shadows": dict(points=True, spots=True, cubes=4),                # light_point_shadows_kernel
    "point_spot_shadows": dict(points=True, spots=True, cubes=4, maps=3),
    "g0_half": dict(points=True, spots=True, cubes=4, maps=3, mix=gf.G0_F16),   # light_general_local_kernel: the cull sees the widened G0
    "gloss": dict(points=True, spots=True, gloss=True),
    "gloss_sh": dict(points=True, spots=True, gloss=True, sh=True),
    "cube_chain": dict(points=True, spots=True, chain=True),                # CubeChain: 32 x 2 pixels per wavefront, the same tile
}


def seeds_of(family):
    """The family's case set: one coherent frame (even seed) and one incoherent (odd)."""
    k = list(FAMILIES).index(family)
    return (2 * k, 2 * k + 1)


class Case:
    """One frame bound for one family.  planes: what the product reads (G0 possibly float16); wide: the same widened to float32
    for the checkers; cb / pcb: the pass constants (with the spot shadow transforms) for the product and the checkers; flags; kw:
    points, spots, maps, cubes, projs, cube_dim as hostsim_lib.run_light takes them; ambient: an ambient map or None."""

    def __init__(self, family, seed, built_lib, n_points=1024, n_spots=1024, lights=None):
        from crychic_renderer_amd import geometry as g
        from test_point_shadows import point_transforms, random_cubes
        f = FAMILIES[family]
        self.family, self.seed = family, seed
        planes, c, knobs, P, S = fuzz_util.light_cull_case(seed, built_lib, n_points, n_spots)
        if lights is not None:
            P, S = lights
        self.W, self.H = fuzz_util.CULL_W, fuzz_util.CULL_H
        self.point_records = P if f.get("points") else P[:0]
        self.spot_records = S if f.get("spots") else S[:0]
        points = fuzz_util.lights_from_records(self.point_records) if len(self.point_records) else None
        spots = fuzz_util.lights_from_records(self.spot_records) if len(self.spot_records) else None
        self.ndl, self.radius = knobs["numDirLights"], knobs["pcfSearchRadius"]
        self.flags = knobs["sky"] | (FIX_ALL if seed & 2 else 0)
        p = {k: planes[k] for k in ("g0", "g1", "g2", "depth", "shadow")}
        cube, self.kw = planes["cube"], {}
        dim = int(cube.shape[1])
        if f.get("chain") or f.get("gloss"):
            cube, levels = g.cube_mip_chain(cube)
            self.flags |= (levels & 15) << 16
            self.kw["cube_dim"] = dim
            if f.get("gloss"):
                self.flags |= gloss_lib.GLOSS
            if f.get("sh"):
                rng = np.random.default_rng(900 + seed)
                cube = env_sh_lib.with_tail(cube, dim, levels, rng.standard_normal((9, 4)).astype(np.float32))
                self.flags |= env_sh_lib.AMBIENT_SH
        p["cube"] = cube
        self.planes = gf.pack_planes(p, f.get("mix", 0))
        self.wide = gf.widen_planes(self.planes)
        self.cb, self.pcb = c.pass_cb, oracle_lib.as_oracle_cb(c.pass_cb, oracle_lib.OrPassConstants)
        if points is not None:
            self.kw["points"] = points
        if spots is not None:
            self.kw["spots"] = spots
        if f.get("maps"):
            self.cb, self.pcb = with_transforms(c.pass_cb, [transposed(st) for _, _, st in spot_transforms(spots, 8)])
            self.kw["maps"] = random_maps(f["maps"], MAP_DIM, 70 + seed)
        if f.get("cubes"):
            self.kw["cubes"] = random_cubes(f["cubes"], CUBE_DIM, 80 + seed)
            self.kw["projs"] = [sp.reshape(-1) for _, _, sp in point_transforms(points, f["cubes"], CUBE_DIM)]
        self.ambient = np.random.default_rng(seed).integers(0, 65536, (self.H // 2, self.W // 2), dtype=np.uint16) if seed & 1 else None
        self._ref = None

    def reference(self):
        """The family's frozen checker on the widened planes, whole frame: (RGBA8, radiance).  Computed once."""
        if self._ref is None:
            f = FAMILIES[self.family]
            if f.get("sh"):
                fn = env_sh_lib.load().checker_light
            elif f.get("gloss"):
                fn = gloss_lib.load().checker_light
            elif not f.get("points"):
                fn = local_light_lib.load().checker
            else:
                fn = point_shadow_lib.load().checker
            self._ref = fn(self.pcb, self.wide, self.ambient, self.ndl, self.radius, self.flags, **self.kw)
        return self._ref

    def host(self, hostsim, tiled, **rows):
        """The product's body on the host: un-culled (RGBA8, radiance) or tiled (RGBA8, radiance, masks)."""
        fn = hostsim.light_frame_tiled if tiled else hostsim.light_frame
        return fn(self.cb, self.planes, self.ambient, self.ndl, self.radius, self.flags, **self.kw, **rows)

    def covered(self):
        return (self.planes["depth"] & 0xFFFFFF) < 0xFFFFFF

    def finite(self):
        return np.isfinite(self.wide["g0"][..., :3]).all(-1)


def mask_bits(masks):
    """(tiles y, tiles x, 2, 1024) booleans from light_frame_tiled's mask words."""
    return np.unpackbits(np.ascontiguousarray(masks).view(np.uint8), bitorder="little").reshape(masks.shape[:3] + (1024,)).astype(bool)


def tile_view(plane, ty, tx, row0=0):
    return plane[row0 + 4 * ty:row0 + 4 * ty + 4, 64 * tx:64 * tx + 64]
