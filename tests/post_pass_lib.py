"""What the test columns of the post-process passes (anti-aliasing, fog, depth of field, decals, bloom, temporal anti-aliasing,
motion blur) share (TEST INFRASTRUCTURE ONLY): the guarded host and device planes, the builds of the C checkers and of the host
builds of the kernel bodies, the device fixture and the tail of every run_device."""
import os
import subprocess

import numpy as np
import pytest

from hostsim_lib import CLANG, CSRC, ROOT

GUARD = 0xA5
GUARD_BYTES = 256       # of GUARD on either side of a device plane


# ---- the host (CPU tier) -----------------------------------------------------------------------------------------------------------

def guarded(shape, dtype=np.uint8, guard=64, misalign=0, fill=GUARD):
    """(raw, view): `view` is an array of `shape` and `dtype` inside the uint8 array `raw` of `fill`, at least `guard` bytes of it on
    either side; the view starts `misalign` bytes (at most 64) past a 64-byte boundary."""
    assert 0 <= misalign <= 64
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.full(n + 2 * guard + 128, fill, np.uint8)
    off = guard + (-(raw.ctypes.data + guard)) % 64 + misalign
    return raw, raw[off:off + n].view(dtype).reshape(shape)


def guards_intact(raw, view, fill=GUARD):
    """Every byte of `raw` outside `view` is `fill`."""
    off = view.ctypes.data - raw.ctypes.data
    return bool((raw[:off] == fill).all() and (raw[off + view.nbytes:] == fill).all())


def _stale(lib, deps):
    return not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps)


def build_checker(src, lib, fp=True):
    """The C checker `lib` from its one source; fp: it computes in floating point (no contraction, libm)."""
    if _stale(lib, [src]):
        subprocess.run(["gcc", "-O2", "-std=c99", "-fPIC", "-Wall"] + (["-ffp-contract=off"] if fp else []) + ["-shared", "-o", lib, src] +
                       (["-lm"] if fp else []), check=True)
    return lib


def build_host_shim(src, lib, headers, api_header=False):
    """The host build `lib` of a kernel body from its one source and csrc's `headers`; api_header: it includes include/crychic_hip.h
    too."""
    include = os.path.join(ROOT, "include")
    deps = [src] + [os.path.join(CSRC, h) for h in headers] + ([os.path.join(include, "crychic_hip.h")] if api_header else [])
    if _stale(lib, deps):
        subprocess.run([CLANG, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma"] +
                       (["-I", include] if api_header else []) + ["-I", CSRC, src, "-o", lib], check=True)
    return lib


# ---- the device (GPU tier) ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev(built_lib):
    """(the product's _lib module, a Context, torch)."""
    import torch
    from crychic_renderer_amd import Context
    ctx = Context(0)
    yield built_lib, ctx, torch
    ctx.close()


def guarded_plane(torch, ctx, host, misalign=0):
    """(raw, view): a device copy of the numpy array `host`, as bytes, inside a uint8 buffer of GUARD, at least GUARD_BYTES of them on
    either side; the view starts `misalign` bytes (at most 256) past a 256-byte boundary."""
    assert 0 <= misalign <= 256
    n = host.nbytes
    raw = torch.full((n + 2 * GUARD_BYTES + 512,), GUARD, dtype=torch.uint8, device=ctx.device)
    off = GUARD_BYTES + (-(raw.data_ptr() + GUARD_BYTES)) % 256 + misalign
    view = raw[off:off + n]
    view.copy_(torch.from_numpy(np.array(host).view(np.uint8).reshape(-1)).to(ctx.device))      # a copy: the corpora are read-only
    return raw, view


def device_guards_intact(raw, view):
    """Every byte of `raw` outside `view` is GUARD."""
    off = view.data_ptr() - raw.data_ptr()
    return bool((raw[:off] == GUARD).all()) and bool((raw[off + view.numel():] == GUARD).all())


class DevicePlanes:
    """The guarded device planes of one call, and what a run_device asserts of them once the call is through."""

    def __init__(self, dev):
        _, self.ctx, self.torch = dev
        self.planes = []        # (name, raw, view, the host array the view must still equal or None)

    def upload(self, name, host, misalign=0, writable=False):
        """The view of a guarded device copy of `host`; unless `writable`, the call under test must leave it as it is."""
        raw, view = guarded_plane(self.torch, self.ctx, host, misalign)
        self.planes.append((name, raw, view, None if writable else host))
        return view

    def blank(self, name, shape, dtype=np.uint8, misalign=0):
        """The view of a guarded device plane of `shape` and `dtype` whose every byte is GUARD, for the call to write."""
        return self.upload(name, np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, GUARD, np.uint8), misalign, writable=True)

    def verify(self):
        for name, raw, view, host in self.planes:
            assert device_guards_intact(raw, view), "guard bytes of the %s plane changed" % name
            assert host is None or np.array_equal(view.cpu().numpy(), np.ascontiguousarray(host).view(np.uint8).reshape(-1)), \
                "the %s plane changed" % name
