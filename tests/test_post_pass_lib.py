"""tests/post_pass_lib.py itself: the guarded planes of the post passes' tests lie where they say, and their checks see every byte
outside the view and none inside it -- on the host, and on the device (no kernel of the product runs: every write is a torch index
assignment into the test's own buffer)."""
import numpy as np
import pytest

import post_pass_lib as pp
from post_pass_lib import dev      # noqa: F401 -- the module's fixture

SHAPE = (3, 5, 4)


@pytest.mark.parametrize("misalign", [0, 4, 8, 12, 16, 32])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32])
def test_guarded_host_plane(dtype, misalign):
    fill = 0x5A
    for kw, f in ((dict(), pp.GUARD), (dict(guard=7, fill=fill), fill)):
        raw, view = pp.guarded(SHAPE, dtype, misalign=misalign, **kw)
        off = view.ctypes.data - raw.ctypes.data
        end = off + view.nbytes
        assert (view.ctypes.data - misalign) % 64 == 0
        assert view.shape == SHAPE and view.dtype == dtype and (view.view(np.uint8) == f).all()
        assert off >= kw.get("guard", 64) and raw.size - end >= kw.get("guard", 64) and (raw == f).all()
        assert pp.guards_intact(raw, view, f)
        for at in (0, off - 1, end, raw.size - 1):            # any single byte outside the view
            raw[at] ^= 0xFF
            assert not pp.guards_intact(raw, view, f), at
            raw[at] ^= 0xFF
        assert pp.guards_intact(raw, view, f)
        for at in (off, end - 1):                             # a byte inside it
            raw[at] ^= 0xFF
            assert pp.guards_intact(raw, view, f), at


def host_plane():
    return np.random.default_rng(26).integers(0, 256, SHAPE, dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [0, 12])
def test_guarded_device_plane(dev, misalign):
    lib, ctx, torch = dev
    host = host_plane()
    raw, view = pp.guarded_plane(torch, ctx, host, misalign)
    off = view.data_ptr() - raw.data_ptr()
    end = off + host.nbytes
    assert (view.data_ptr() - misalign) % 256 == 0
    assert off >= pp.GUARD_BYTES and raw.numel() - end >= pp.GUARD_BYTES
    assert np.array_equal(view.cpu().numpy().reshape(SHAPE), host)
    assert pp.device_guards_intact(raw, view)
    for at in (off - 1, end):
        raw[at] = pp.GUARD ^ 0xFF
        assert not pp.device_guards_intact(raw, view), at
        raw[at] = pp.GUARD
    raw[off] = int(host.reshape(-1)[0]) ^ 0xFF                 # a byte inside the view
    assert pp.device_guards_intact(raw, view)


@pytest.mark.gpu
def test_device_planes_verify_names_the_plane(dev):
    host = host_plane()
    planes = pp.DevicePlanes(dev)
    src = planes.upload("input", host, 12)
    io = planes.upload("in place", host, 4, writable=True)
    out = planes.blank("out", SHAPE, np.uint16, 8)
    assert out.numel() == 2 * host.size and bool((out == pp.GUARD).all())
    io[3] = int(host.reshape(-1)[3]) ^ 0xFF                    # writable planes may change
    out[0] = 0
    planes.verify()
    src[7] = int(host.reshape(-1)[7]) ^ 0xFF
    with pytest.raises(AssertionError, match="the input plane changed"):
        planes.verify()
    src[7] = int(host.reshape(-1)[7])
    planes.verify()
    raw, view = next((r, v) for name, r, v, _ in planes.planes if name == "out")
    at = view.data_ptr() - raw.data_ptr() + view.numel()      # the first byte behind the view
    raw[at] = 0
    with pytest.raises(AssertionError, match="guard bytes of the out plane changed"):
        planes.verify()
