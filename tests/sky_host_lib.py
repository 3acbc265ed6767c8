"""Builds and loads tests/sky_host (TEST INFRASTRUCTURE ONLY): csrc/sky_core.hpp, the body of sky_kernel and of
crychic_sky_sun_colour, compiled for the host with the workgroup and lane walk emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import sky_lib

DIR = os.path.join(ROOT, "tests", "sky_host")
SRC, LIB = os.path.join(DIR, "sky_host.cpp"), os.path.join(DIR, "libskyhost.so")
HEADERS = ("sky_core.hpp", "devmath.hpp", "gamma_pow.inc")


def build():
    return build_host_shim(SRC, LIB, HEADERS)


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.skh_render_sky.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _LIB.skh_render_sky.restype = C.c_uint32
        _LIB.skh_sun_colour.argtypes = [C.c_void_p, C.c_void_p]
        _LIB.skh_sun_colour.restype = None
    return _LIB


def render_sky(cube, dim, params=None, face0=0, faces=6):
    """Level 0 of faces [face0, face0 + faces) of the (6, dim, dim, 4) uint8 cube `cube` (contiguous, used in place) as the kernel
    body writes them.  Returns the number of workgroups walked."""
    assert cube.flags.c_contiguous and cube.dtype == np.uint8 and cube.shape == (6, dim, dim, 4)
    p = sky_lib.params_array(params)
    return _lib().skh_render_sky(cube.ctypes.data, dim, face0, faces, p.ctypes.data)


def sun_colour(params=None):
    rgb = np.zeros(3, np.float32)
    p = sky_lib.params_array(params)
    _lib().skh_sun_colour(p.ctypes.data, rgb.ctypes.data)
    return rgb
