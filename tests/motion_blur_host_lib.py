"""Builds and loads tests/motion_blur_host (TEST INFRASTRUCTURE ONLY): csrc/motion_blur_core.hpp, the bodies of the two motion blur
kernels, compiled for the host with the workgroup and lane walk emulated."""
import ctypes as C
import os

import numpy as np

from hostsim_lib import ROOT
from post_pass_lib import build_host_shim
import motion_blur_lib as mbl

DIR = os.path.join(ROOT, "tests", "motion_blur_host")
SRC, LIB = os.path.join(DIR, "motion_blur_host.cpp"), os.path.join(DIR, "libmotionblurhost.so")


def build():
    return build_host_shim(SRC, LIB, ("motion_blur_core.hpp", "devmath.hpp", "gamma_pow.inc"))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.mbh_velocity.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_void_p]
        _LIB.mbh_velocity.restype = C.c_uint32
        _LIB.mbh_gather.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 5 + [C.c_void_p]
        _LIB.mbh_gather.restype = C.c_uint32
        _LIB.mbh_workspace_bytes.argtypes = [C.c_uint32] * 2
        _LIB.mbh_workspace_bytes.restype = C.c_uint64
    return _LIB


def workspace_bytes(W, H):
    return int(_lib().mbh_workspace_bytes(W, H))


def velocity(case, ws=None):
    """(workspace, workgroups walked): the workspace as the velocity kernel's body writes it, into 0xA5 bytes by default."""
    ws = np.full(mbl.workspace_bytes(case.W, case.H), mbl.GUARD, np.uint8) if ws is None else ws
    groups = _lib().mbh_velocity(case.ivp.ctypes.data, case.cur.ctypes.data, case.prev.ctypes.data, case.depth.ctypes.data, case.W, case.H, case.shutter,
                                 case.radius, ws.ctypes.data)
    return ws, groups


def gather(case, ws, row0=0, rows=None, out=None, img=None):
    """(out, workgroups walked): rows [row0, row0 + rows) as the gather kernel's body writes them, into a plane of 0xA5 bytes by default."""
    H, W = case.H, case.W
    rows = H - row0 if rows is None else rows
    out = np.full((H, W, 4), mbl.GUARD, np.uint8) if out is None else out
    img = case.img if img is None else np.ascontiguousarray(img, np.uint8)
    groups = _lib().mbh_gather(img.ctypes.data, out.ctypes.data, W, H, row0, rows, case.samples, ws.ctypes.data)
    return out, groups
