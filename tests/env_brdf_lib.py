"""Builds and loads the checker and the host harness of the environment BRDF table and of the lighting pass's split-sum reflection
weight (TEST INFRASTRUCTURE ONLY): tests/env_brdf_ref/libenvbrdfref.so -- tests/env_sh_ref/env_sh_ref.c included unchanged, with the
table and the lighting pixel restated, built with the oracle's flags -- and tests/env_brdf_host/libenvbrdfhost.so,
csrc/env_brdf_core.hpp and the lighting call with SpecularSplitSum (tests/hostsim/host_light.hpp, bound through light_bind.hpp) compiled for
the host.
Both are rebuilt when a source is newer.  With CRYCHIC_SANITIZE=1 the harness is the ASan + UBSan build."""
import ctypes as C
import os

import numpy as np

import env_sh_lib
import gloss_lib
import local_light_lib
import point_shadow_lib
import hostsim_lib
from hostsim_lib import LIGHT_ARGTYPES, ROOT, run_light

ENV_BRDF = 0x100000     # CRYCHIC_LIGHT_ENV_BRDF
TABLE_BYTES = 4096      # CRYCHIC_ENV_BRDF_BYTES
TAIL_BYTES = env_sh_lib.TAIL_BYTES

REF_DIR, HOST_DIR = os.path.join(ROOT, "tests", "env_brdf_ref"), os.path.join(ROOT, "tests", "env_brdf_host")
REF_SRC, REF_LIB = os.path.join(REF_DIR, "env_brdf_ref.c"), os.path.join(REF_DIR, "libenvbrdfref.so")
HOST_SRC, HOST_LIB = os.path.join(HOST_DIR, "env_brdf_host.cpp"), os.path.join(HOST_DIR, "libenvbrdfhost.so")


def build_ref():
    return local_light_lib.build_checker(REF_LIB, [REF_SRC, env_sh_lib.REF_SRC, gloss_lib.REF_SRC, point_shadow_lib.REF_SRC,
                                                   local_light_lib.REF_SRC])


def build_host():
    return hostsim_lib.build_host(HOST_LIB, HOST_SRC, ("env_brdf_core.hpp",))


def build():
    return build_ref(), build_host()


def table_offset(dim, levels):
    """crychic_cube_env_brdf_offset, restated."""
    return env_sh_lib.tail_offset(dim, levels) + TAIL_BYTES


def with_table(cube, dim, levels, table, coeffs=None, fill=0xA5):
    """A flat uint8 array: the chain `cube`, padding to 16 bytes, the 512-byte environment tail (its first 144 bytes the (9, 4)
    float32 `coeffs` if given) and the 1024 uint32 of `table`; every other byte of padding and tail is `fill`."""
    n, off = env_sh_lib.chain_bytes(dim, levels), table_offset(dim, levels)
    out = np.full(off + TABLE_BYTES, fill, np.uint8)
    out[:n] = np.ascontiguousarray(cube, np.uint8).reshape(-1)[:n]
    if coeffs is not None:
        out[off - TAIL_BYTES:off - TAIL_BYTES + 144] = np.ascontiguousarray(coeffs, np.float32).reshape(-1).view(np.uint8)
    out[off:] = np.ascontiguousarray(table, np.uint32).reshape(-1).view(np.uint8)
    return out


class EnvBrdfLib:
    def __init__(self):
        ref, host = build()
        self._ref, self._host = C.CDLL(ref), C.CDLL(host)
        vp, u32 = C.c_void_p, C.c_uint32
        self._ref.eb_sums.argtypes = [u32, u32, u32, u32, vp]
        self._ref.eb_sums.restype = C.c_float
        self._ref.eb_pack.argtypes = [vp]
        self._ref.eb_pack.restype = u32
        self._ref.eb_table.argtypes = [vp, vp]
        self._ref.eb_lookup.argtypes = [vp, C.c_float, C.c_float, vp]
        self._ref.eb_lookup.restype = None
        self._ref.eb_r0.argtypes = [vp, C.c_float, vp]
        self._ref.eb_r0.restype = None
        self._ref.eb_table_offset.argtypes = [u32, u32]
        self._ref.eb_table_offset.restype = C.c_size_t
        self._host.bh_sums.argtypes = [u32, u32, vp, u32, vp]
        self._host.bh_sums.restype = None
        self._host.bh_build.argtypes = [vp, vp]
        self._host.bh_build.restype = None
        self._host.bh_pack.argtypes = [vp]
        self._host.bh_pack.restype = u32
        self._host.bh_table_offset.argtypes = [u32, u32]
        self._host.bh_table_offset.restype = C.c_uint64
        self._host.bh_check.argtypes = [u32, C.c_size_t, u32]
        self._host.bh_check_message.argtypes = [u32, C.c_size_t, u32, C.c_char_p, C.c_size_t]
        self._ref.eb_deferred_light_spec.argtypes = LIGHT_ARGTYPES
        self._host.bh_light.argtypes = LIGHT_ARGTYPES
        self._host.bh_light.restype = C.c_int
        self._table = None

    def ref_sums(self, j, i, first=0, last=4096):
        """(the checker's two int64 sums of texel (j, i) over samples [first, last), the largest term met or -1)."""
        s = np.zeros(2, np.int64)
        worst = self._ref.eb_sums(j, i, first, last, s.ctypes.data)
        return s, worst

    def host_sums(self, j, i, rows):
        """The kernel body's two sums over the xi rows listed, in that order."""
        r = np.ascontiguousarray(rows, np.uint32)
        s = np.zeros(2, np.int64)
        self._host.bh_sums(j, i, r.ctypes.data, r.size, s.ctypes.data)
        return s

    def table(self):
        """The checker's (1024 uint32 dwords, (1024, 2) int64 sums); its bounds hold (eb_table returned 0).  Computed once."""
        if self._table is None:
            t, s = np.zeros(1024, np.uint32), np.zeros((1024, 2), np.int64)
            assert self._ref.eb_table(t.ctypes.data, s.ctypes.data) == 0, "a bound of the definition does not hold"
            t.setflags(write=False); s.setflags(write=False)
            self._table = (t, s)
        return self._table

    def host_table(self, fill=0xFF):
        """The kernel body's (dwords, sums), the destination pre-filled with `fill`."""
        t, s = np.full(1024, fill * 0x01010101, np.uint32), np.zeros((1024, 2), np.int64)
        self._host.bh_build(t.ctypes.data, s.ctypes.data)
        return t, s

    def lookup(self, table, n_dot_v, roughness):
        ab = np.zeros(2, np.float32)
        self._ref.eb_lookup(np.ascontiguousarray(table, np.uint32).ctypes.data, n_dot_v, roughness, ab.ctypes.data)
        return ab

    def r0(self, albedo, metalness):
        a, r = np.ascontiguousarray(albedo, np.float32), np.zeros(3, np.float32)
        self._ref.eb_r0(a.ctypes.data, metalness, r.ctypes.data)
        return r

    def checker_light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights):
        """The checker's frame (RGBA8, radiance) with CRYCHIC_LIGHT_ENV_BRDF: p["cube"] is with_table's array; float32 planes."""
        return run_light(self._ref.eb_deferred_light_spec, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def host_light(self, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights):
        """The same call through the kernel body on the host (bh_light); formats=True: planes in their own dtypes."""
        return run_light(self._host.bh_light, cb, p, ambient, num_dir_lights, pcf_radius, flags, **lights)

    def check(self, flags, cube_address, cube_dim):
        """light_bind.hpp's env_brdf_check: 0 ok, 1 no gloss chain, 2 null cube map, 3 misaligned table."""
        return self._host.bh_check(flags, cube_address, cube_dim)

    def check_message(self, flags, cube_address, cube_dim):
        """The message the entries report that refusal with (api.cpp formats light_bind.hpp's text); empty when the call is valid."""
        buf = C.create_string_buffer(256)
        self._host.bh_check_message(flags, cube_address, cube_dim, buf, len(buf))
        return buf.value.decode()


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = EnvBrdfLib()
    return _LIB
