"""The CPU tier of the devmath ladder: every primitive of csrc/devmath.hpp compiled for the host (tests/hostsim hs_eval_array)
against the oracle's definition of it (or_eval_array), bit for bit, on the inputs of tests/devmath_dev_lib.py -- exhaustive for
the 16- and 24-bit formats, elsewhere a lattice of 2^24 patterns (every upper half-word, 256 lower ones) plus the algorithms'
breakpoints +- 8 ulp.  tests/test_devmath_gpu.py runs the same arrays through the device build, whose `__HIP_DEVICE_COMPILE__`
branches this tier cannot see.  No tolerance anywhere: bit equality, any NaN equal to any NaN, and the share of NaN results -- which
that rule is blind on -- is capped per kind."""
import numpy as np
import pytest

import devmath_dev_lib as dm


@pytest.mark.parametrize("name", sorted(dm.CASES))
def test_host_build_equals_the_definition(hostsim, oracle, name):
    case = dm.CASES[name]()
    assert case.a.size == case.kept, (name, case.a.size, case.kept)                # the domain's predicate kept what it should
    a, b = dm.u2f(case.a), None if case.b is None else dm.u2f(case.b)
    ref = oracle.eval_array(case.kind, a, b)
    got = hostsim.eval_array(case.kind, a, b)
    bad = dm.same_results(case, got, ref)
    print("%s: %d inputs compared, %d differ" % (name, case.a.size, bad))
    assert bad == 0, (name, bad)
    if case.cap is not None:
        share = dm.nan_share(ref)
        print("%s: NaN share of the definition's results %.4f %% (cap %.1f %%)" % (name, 100.0 * share, 100.0 * case.cap))
        assert share <= case.cap, (name, share)
    if dm.FULL and name in dm.UNARY_FULL:          # the soak run: all 2^32 patterns, in chunks of 2^24
        for a, b in dm.full_chunks(name):
            assert dm.same_results(case, hostsim.eval_array(case.kind, a, b), oracle.eval_array(case.kind, a, b)) == 0, (name, a.view(np.uint32)[0])


def test_lattice_is_what_it_says():
    lat = dm.lattice()
    assert lat.size == 1 << 24 and np.unique(lat).size == 1 << 24
    assert np.array_equal(np.unique(lat >> 16), np.arange(65536))                  # every upper half-word: exponents, signs, specials
    low = set(int(x) for x in dm.lower_halves())
    assert len(low) == 256 and {0x0000, 0x0001, 0x7FFF, 0x8000, 0xFFFF} <= low
    nan = dm.is_nan(lat)
    assert abs(nan.mean() - 0.0039) < 1e-4                                         # the 0.39 % behind the caps
    assert dm.is_snan(lat).sum() == 2 * (255 + 63 * 256) and (nan & ~dm.is_snan(lat)).any()
    assert np.isin(np.array([0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF], np.uint32), lat).all()      # infinities, subnormals
    bp = dm.breakpoints()
    for v in (np.float32(np.pi / 2), np.float32(4096 * np.pi / 2), np.float32(8388608.0), np.float32(0.5 / 255), np.float32(126.5), np.float32(-125.0)):
        assert dm.f2u(v)[0] in bp[np.searchsorted(bp, dm.f2u(v)[0]):][:1]
    assert 0x3F3504F3 in bp[np.searchsorted(bp, 0x3F3504F3):][:1] and 0x3F3504F3 + 8 in bp[np.searchsorted(bp, 0x3F3504F3 + 8):][:1]
