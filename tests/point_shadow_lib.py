"""Builds and loads the shadowed point-light checker (TEST INFRASTRUCTURE ONLY): tests/point_shadow_ref/libpointshadowref.so,
tests/local_light_ref/local_light_ref.c included unchanged, with the cube face step and a shadowed point term, built with the
oracle's flags and rebuilt when a source is newer.  The product's body it is compared with is tests/hostsim's (hostsim_lib)."""
import ctypes as C
import os

import numpy as np

import local_light_lib
import local_lights_util
from hostsim_lib import LIGHT_ARGTYPES, ROOT, run_light

DIR = os.path.join(ROOT, "tests", "point_shadow_ref")
REF_SRC, REF_LIB = os.path.join(DIR, "point_shadow_ref.c"), os.path.join(DIR, "libpointshadowref.so")


def build():
    return local_light_lib.build_checker(REF_LIB, [REF_SRC, local_light_lib.REF_SRC])


class PointShadowLib:
    def __init__(self):
        self._ref = C.CDLL(build())
        vp, u32 = C.c_void_p, C.c_uint32
        self._ref.ps_deferred_light_point_shadows.argtypes = LIGHT_ARGTYPES
        self._ref.ps_point_shadow_factor.argtypes = [vp, u32, vp, vp, vp]
        self._ref.ps_point_shadow_factor.restype = C.c_float
        self._ref.ps_point_face.argtypes = [vp, vp]
        self._ref.ps_point_face.restype = C.c_int

    def checker(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, **lights):
        """The checker's frame (RGBA8, radiance): local_light_lib's checker plus cubes, (count, 6, dim, dim) uint32 D24 faces of the
        first `count` point lights, and projs, their (count, 16) untransposed shadow projections.  cubes None: no point shadows."""
        return run_light(self._ref.ps_deferred_light_point_shadows, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def factor(self, faces, proj, light_pos, pos):
        """The checker's cube shadow factor s of one position; faces (6, dim, dim)."""
        faces = np.ascontiguousarray(faces, np.uint32)
        proj = np.ascontiguousarray(proj, np.float32).reshape(16)
        lp = np.ascontiguousarray(light_pos, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        return self._ref.ps_point_shadow_factor(faces.ctypes.data, faces.shape[1], proj.ctypes.data, lp.ctypes.data, pos.ctypes.data)

    def face(self, v):
        """(f, (a, b, c)) of the checker's face step."""
        v = np.ascontiguousarray(v, np.float32)
        abc = np.zeros(3, np.float32)
        return self._ref.ps_point_face(v.ctypes.data, abc.ctypes.data), abc

# ---- what the tests of the family share: transforms, faces and the descriptors of a device call -----------------------------------
def point_transforms(lights, count, dim, z_near=0.5):
    """crychic_update_point_shadow_transforms of the first `count` lights: [(views (6, 4, 4), proj (4, 4), shadowProj (4, 4))]."""
    from crychic_renderer_amd import lib
    out = []
    for k in range(count):
        lv, lp, sp = ((C.c_float * 16) * 6)(), (C.c_float * 16)(), (C.c_float * 16)()
        assert lib.crychic_update_point_shadow_transforms(C.byref(lights[k]), dim, z_near, lv, lp, sp) == 0
        out.append((np.array([lv[f][:] for f in range(6)], np.float32).reshape(6, 4, 4), np.asarray(lp[:], np.float32).reshape(4, 4),
                    np.asarray(sp[:], np.float32).reshape(4, 4)))
    return out


def random_cubes(count, dim, seed):
    return local_lights_util.random_maps(count * 6, dim, seed).reshape(count, 6, dim, dim)


def spot_desc(dev_maps, count=None):
    from crychic_renderer_amd._lib import SpotShadows
    d = SpotShadows()
    if dev_maps is not None:
        d.count = dev_maps.shape[0] if count is None else count
        d.dim = dev_maps.shape[1]
        for k in range(dev_maps.shape[0]):
            d.maps[k] = dev_maps[k].data_ptr()
    return d


def point_desc(dev_cubes, projs=None, count=None):
    from crychic_renderer_amd._lib import PointShadows
    d = PointShadows()
    if dev_cubes is not None:
        d.count = dev_cubes.shape[0] if count is None else count
        d.dim = dev_cubes.shape[2]
        for k in range(dev_cubes.shape[0]):
            d.maps[k] = dev_cubes[k].data_ptr()
            d.shadowProj[k][:] = [float(v) for v in np.asarray(projs[k], np.float32).reshape(-1)]
    return d


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = PointShadowLib()
    return _LIB
