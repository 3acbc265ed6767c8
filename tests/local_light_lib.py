"""Builds and loads the local-light checker (TEST INFRASTRUCTURE ONLY): tests/local_light_ref/liblocallightref.so, the frozen
oracle's or_light.c with the spot loop and a shadow factor per spot light, built with the oracle's flags and rebuilt when a source
is newer.  The product's body it is compared with is tests/hostsim's (hostsim_lib), which also owns the marshalling of a call."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import LIGHT_ARGTYPES, ROOT, run_light

DIR = os.path.join(ROOT, "tests", "local_light_ref")
ORACLE = os.path.join(ROOT, "oracle")
REF_SRC, REF_LIB = os.path.join(DIR, "local_light_ref.c"), os.path.join(DIR, "liblocallightref.so")
# oracle/Makefile's CFLAGS: -ffp-contract=off is part of the definition
ORACLE_FLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-fopenmp", "-Wall", "-Wextra",
                "-Wno-unused-parameter", "-Wno-unused-function"]
ORACLE_DEPS = [os.path.join(ORACLE, f) for f in ("or_light.c", "crychic_oracle.h", "or_math.h", "or_samplers.h", "or_gamma_pow.inc")]


def build_checker(lib, sources):
    """gcc with the oracle's flags over sources[0] (the others are what it includes), when one of them is newer than lib."""
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in list(sources) + ORACLE_DEPS):
        subprocess.run(["gcc"] + ORACLE_FLAGS + ["-I", ORACLE, "-shared", "-o", lib, sources[0], "-lm"], check=True)
    return lib


def build():
    return build_checker(REF_LIB, [REF_SRC])


class LocalLightLib:
    def __init__(self):
        self._ref = C.CDLL(build())
        self._ref.ss_deferred_light_spots_shadowed.argtypes = LIGHT_ARGTYPES[:26]
        self._ref.ss_spot_shadow_factor.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self._ref.ss_spot_shadow_factor.restype = C.c_float

    def checker(self, cb, p, ambient, num_dir_lights, pcf_radius, flags=0, **lights):
        """The checker's frame (RGBA8, radiance).  cb: an oracle_lib.OrPassConstants (with the spot transforms in
        ShadowTransforms[4 + k] when there are maps); flags: the oracle's word (bit 0 sky, CRYCHIC_FIX_Q*, CRYCHIC_LIGHT_CUBE_LEVELS);
        lights: points / spots, ctypes arrays of Light or None; maps, (count, dim, dim) uint32 D24 maps of the first `count` spot
        lights, or None for unshadowed spot lights; row0, rows, cube_dim."""
        return run_light(self._ref.ss_deferred_light_spots_shadowed, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def factor(self, m, T, pos):
        """The checker's shadow factor s of one position."""
        m = np.ascontiguousarray(m, np.uint32)
        T = np.ascontiguousarray(T, np.float32)
        pos = np.ascontiguousarray(pos, np.float32)
        return self._ref.ss_spot_shadow_factor(m.ctypes.data, m.shape[0], T.ctypes.data, pos.ctypes.data)


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = LocalLightLib()
    return _LIB
