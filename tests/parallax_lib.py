"""Builds and loads the checker and the host harness of the box-projected reflection lookup (TEST INFRASTRUCTURE ONLY):
tests/parallax_ref/libparallaxref.so -- tests/env_brdf_ref/env_brdf_ref.c included unchanged, with the correction and the lighting
pixel restated, built with the oracle's flags -- and tests/parallax_host/libparallaxhost.so, light_core.hpp's probe_project and the
lighting call with CubeGlossBox (tests/parallax_host/host_light_probe.hpp, bound through light_bind.hpp) compiled for the host.
Both are rebuilt when a source is newer.  With CRYCHIC_SANITIZE=1 the harness is the ASan + UBSan build."""
import ctypes as C
import os

import numpy as np

import env_brdf_lib
import env_sh_lib
import gloss_lib
import local_light_lib
import point_shadow_lib
import hostsim_lib
from hostsim_lib import LIGHT_ARGTYPES, ROOT, run_light

PARALLAX = 0x200000     # CRYCHIC_LIGHT_CUBE_PARALLAX
PROBE_OFFSET, PROBE_BYTES = 368, 48     # CRYCHIC_CUBE_PROBE_OFFSET, CRYCHIC_CUBE_PROBE_BYTES
TAIL_BYTES = env_sh_lib.TAIL_BYTES

REF_DIR, HOST_DIR = os.path.join(ROOT, "tests", "parallax_ref"), os.path.join(ROOT, "tests", "parallax_host")
REF_SRC, REF_LIB = os.path.join(REF_DIR, "parallax_ref.c"), os.path.join(REF_DIR, "libparallaxref.so")
HOST_SRC, HOST_LIB = os.path.join(HOST_DIR, "parallax_host.cpp"), os.path.join(HOST_DIR, "libparallaxhost.so")
HOST_LOOP = os.path.join(HOST_DIR, "host_light_probe.hpp")


def build_ref():
    return local_light_lib.build_checker(REF_LIB, [REF_SRC, env_brdf_lib.REF_SRC, env_sh_lib.REF_SRC, gloss_lib.REF_SRC, point_shadow_lib.REF_SRC,
                                                   local_light_lib.REF_SRC])


def build_host():
    # the harness's own pixel loop is a dependency build_host does not know: a library older than it is built again
    for lib in (HOST_LIB, os.path.join(hostsim_lib.SAN_DIR, os.path.basename(HOST_LIB))):
        if os.path.exists(lib) and os.path.getmtime(HOST_LOOP) > os.path.getmtime(lib):
            os.remove(lib)
    return hostsim_lib.build_host(HOST_LIB, HOST_SRC, ())


def build():
    return build_ref(), build_host()


def probe_offset(dim, levels):
    """crychic_cube_probe_offset, restated."""
    return env_sh_lib.tail_offset(dim, levels) + PROBE_OFFSET


def probe_floats(pos, box_min, box_max):
    """The twelve floats of a probe volume: c, bmin, bmax as float4 with w = 0."""
    v = np.zeros((3, 4), np.float32)
    v[0, :3], v[1, :3], v[2, :3] = pos, box_min, box_max
    return v.reshape(-1)


def with_probe(cube, dim, levels, probe, coeffs=None, table=None, fill=0xA5):
    """A flat uint8 array: the chain `cube`, padding to 16 bytes, the 512-byte environment tail -- its first 144 bytes the (9, 4)
    float32 `coeffs` if given, bytes [368, 416) the twelve floats `probe` -- and, if given, the 1024 uint32 of `table` behind it;
    every other byte of padding and tail is `fill`."""
    n, off = env_sh_lib.chain_bytes(dim, levels), env_sh_lib.tail_offset(dim, levels)
    out = np.full(off + TAIL_BYTES + (env_brdf_lib.TABLE_BYTES if table is not None else 0), fill, np.uint8)
    out[:n] = np.ascontiguousarray(cube, np.uint8).reshape(-1)[:n]
    if coeffs is not None:
        out[off:off + 144] = np.ascontiguousarray(coeffs, np.float32).reshape(-1).view(np.uint8)
    out[off + PROBE_OFFSET:off + PROBE_OFFSET + PROBE_BYTES] = np.ascontiguousarray(probe, np.float32).reshape(-1).view(np.uint8)
    if table is not None:
        out[off + TAIL_BYTES:] = np.ascontiguousarray(table, np.uint32).reshape(-1).view(np.uint8)
    return out


class ParallaxLib:
    def __init__(self):
        ref, host = build()
        self._ref, self._host = C.CDLL(ref), C.CDLL(host)
        vp, u32 = C.c_void_p, C.c_uint32
        self._ref.px_correct.argtypes = [vp, vp, vp, vp, vp]
        self._ref.px_correct.restype = None
        self._ref.px_probe_offset.argtypes = [u32, u32]
        self._ref.px_probe_offset.restype = C.c_size_t
        self._host.xh_correct_many.argtypes = [vp, vp, vp, vp, C.c_size_t]
        self._host.xh_correct_many.restype = None
        self._host.xh_probe_offset.argtypes = [u32, u32]
        self._host.xh_probe_offset.restype = C.c_uint64
        self._host.xh_check.argtypes = [u32, C.c_size_t, u32]
        self._host.xh_check_message.argtypes = [u32, C.c_size_t, u32, C.c_char_p, C.c_size_t]
        self._host.xh_volume_valid.argtypes = [vp, vp, vp]
        self._host.xh_old_visit.argtypes = [u32]
        self._ref.px_deferred_light_parallax.argtypes = LIGHT_ARGTYPES
        self._host.xh_light.argtypes = LIGHT_ARGTYPES
        self._host.xh_light.restype = C.c_int

    def ref_correct(self, p, r, probe):
        """The checker's (r', t) of each row of p, r (n, 3) under each row of probe (n, 12)."""
        p, r, probe = (np.ascontiguousarray(a, np.float32) for a in (p, r, probe))
        out, t = np.zeros_like(p), np.zeros(len(p), np.float32)
        for i in range(len(p)):
            self._ref.px_correct(p[i].ctypes.data, r[i].ctypes.data, probe[i].ctypes.data, out[i].ctypes.data, t[i:].ctypes.data)
        return out, t

    def host_correct(self, p, r, probe):
        """The kernel body's r' of the same."""
        p, r, probe = (np.ascontiguousarray(a, np.float32) for a in (p, r, probe))
        out = np.zeros_like(p)
        self._host.xh_correct_many(p.ctypes.data, r.ctypes.data, probe.ctypes.data, out.ctypes.data, len(p))
        return out

    def checker_light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights):
        """The checker's frame (RGBA8, radiance) with CRYCHIC_LIGHT_CUBE_PARALLAX: p["cube"] is with_probe's array; float32 planes."""
        assert flags & PARALLAX
        return run_light(self._ref.px_deferred_light_parallax, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def host_light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights):
        """The same call, with or without the flag, through the kernel body on the host (xh_light); formats=True: planes in their own
        dtypes.  Raises if the harness refuses the call."""
        rc = []

        def fn(*a):
            rc.append(self._host.xh_light(*a))
        fn.argtypes = LIGHT_ARGTYPES
        out = run_light(fn, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)
        if rc != [0]:
            raise RuntimeError("xh_light refused the call (flags %#x)" % flags)
        return out

    def host_light_rc(self, cb, p, flags, **lights):
        """xh_light's return value for a one-light call: 0 served, -1 refused."""
        rc = []

        def fn(*a):
            rc.append(self._host.xh_light(*a))
        fn.argtypes = LIGHT_ARGTYPES
        run_light(fn, cb, p, None, 1, 0.0, flags, **lights)
        return rc[0]

    def check(self, flags, cube_address, cube_dim):
        """light_bind.hpp's parallax_check: 0 ok, 1 no gloss chain, 2 null cube map, 3 misaligned probe volume."""
        return self._host.xh_check(flags, cube_address, cube_dim)

    def check_message(self, flags, cube_address, cube_dim):
        """The message the entries report that refusal with (api.cpp formats light_bind.hpp's text); empty when the call is valid."""
        buf = C.create_string_buffer(256)
        self._host.xh_check_message(flags, cube_address, cube_dim, buf, len(buf))
        return buf.value.decode()

    def volume_valid(self, pos, box_min, box_max):
        """light_bind.hpp's probe_volume_valid, the setter's check of its values."""
        a = [np.ascontiguousarray(v, np.float32) for v in (pos, box_min, box_max)]
        return bool(self._host.xh_volume_valid(*[v.ctypes.data for v in a]))

    def old_visit(self, flags):
        """How often tests/hostsim/host_light.hpp's three-policy visit calls its functor for the flags: 1, or 0 when it returns false."""
        return self._host.xh_old_visit(flags)


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = ParallaxLib()
    return _LIB
