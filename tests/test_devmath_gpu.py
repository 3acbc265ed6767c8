"""The device tier of the devmath ladder: every primitive of csrc/devmath.hpp evaluated ON THE DEVICE (tests/devmath_dev, built
with the product's flag set) against the oracle's definition of it, bit for bit, on the arrays tests/test_devmath_lattice_host.py
runs through the host build.  This is the only place where the `__HIP_DEVICE_COMPILE__` branches (v_rcp_f32 / v_sqrt_f32 /
v_rsq_f32 + correction, v_med3_f32, v_mul_u32_u24) and the amdgcn lowering of rintf, ldexpf, floorf, the float -> integer
conversions, fminf / fmaxf on NaN, the constant table and _Float16 meet the definitions outside a whole frame.  No tolerance: bit
equality, any NaN equal to any NaN; the stated domains are predicates on the input, and each case asserts how many inputs it kept."""
import numpy as np
import pytest

import devmath_dev_lib as dm


def test_device_harness_cross_compiles():
    import os
    assert os.path.exists(dm.build())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(dm.CASES))
def test_device_equals_the_definition(built_lib, oracle, name):
    dev = dm.load()
    case = dm.CASES[name]()
    assert case.a.size == case.kept, (name, case.a.size, case.kept)
    a, b = dm.u2f(case.a), None if case.b is None else dm.u2f(case.b)
    ref = oracle.eval_array(case.kind, a, b)
    got = dev.eval_array(case.kind, a, b)
    bad = dm.same_results(case, got, ref)
    print("%s: %d inputs compared, %d differ" % (name, case.a.size, bad))
    if bad:
        g, r = got.view(np.uint32), ref.view(np.uint32)
        k = np.nonzero(g != r)[0][:8] if case.integer else np.nonzero((dm.is_nan(g) != dm.is_nan(r)) | (~dm.is_nan(g) & (g != r)))[0][:8]
        print("   e.g. " + ", ".join("%08x%s -> %08x, the definition %08x" % (case.a[i], "" if case.b is None else " %08x" % case.b[i], g[i], r[i]) for i in k))
    assert bad == 0, (name, bad)
    if dm.FULL and name in dm.UNARY_FULL:          # the soak run: all 2^32 patterns, in chunks of 2^24
        for x, y in dm.full_chunks(name):
            assert dm.same_results(case, dev.eval_array(case.kind, x, y), oracle.eval_array(case.kind, x, y)) == 0, (name, x.view(np.uint32)[0])


@pytest.mark.gpu
def test_device_harness_refuses_what_it_cannot_run(built_lib):
    """More than 2^24 elements, no elements, a kind it does not have, a null pointer: an error code, no launch."""
    dev = dm.load()
    a = np.zeros((1 << 24) + 1, np.float32)
    out = np.full(a.shape, 7.0, np.float32)
    assert dev.eval_raw(dm.RCP, a, a, out) != 0
    assert dev.eval_raw(dm.RCP, a[:0], a[:0], out[:0]) != 0
    for kind in (-1, dm.NRAND, 52, 1 << 20):
        assert dev.eval_raw(kind, a[:16], a[:16], out[:16]) != 0, kind
    assert dev.lib.dm_eval_array(dm.RCP, 16, None, a.ctypes.data, out.ctypes.data) != 0
    assert (out == 7.0).all()
    assert dev.eval_raw(dm.RCP, a[:16] + 2.0, a[:16], out[:16]) == 0 and (out[:16] == 0.5).all()
