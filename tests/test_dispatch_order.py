"""The dispatch-order map of the SSAO and lighting launches (csrc/dispatch_order.hpp), on the host: the header is built into a small
shim with the host compiler and the map is checked to be a permutation -- a band that no workgroup covers, or that two cover, is
the only way a placement can change a pixel."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "dispatch_order_ref")
CSRC = os.path.join(ROOT, "crychic_renderer_amd", "csrc")
SRC, LIB = os.path.join(DIR, "dispatch_order_shim.cpp"), os.path.join(DIR, "libdispatchorder.so")
WAYS = (0, 1, 2, 3, 4, 8)


def build_shim(lib=LIB, defs=()):
    deps = [SRC, os.path.join(CSRC, "dispatch_order.hpp")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-I", CSRC, *defs, "-o", lib, SRC],
                       check=True)
    s = C.CDLL(lib)
    for name, n in (("shim_band_of", 3), ("shim_launch_band", 3), ("shim_light_dispatch_row", 2), ("shim_light_band_rows", 0),
                    ("shim_light_ways", 0), ("shim_ssao_ways", 0)):
        f = getattr(s, name)
        f.argtypes, f.restype = [C.c_uint32] * n, C.c_uint32
    return s


@pytest.fixture(scope="module")
def shim():
    return build_shim()


@pytest.mark.parametrize("ways", WAYS)
def test_band_of_is_a_bijection(shim, ways):
    for f in (shim.shim_band_of, shim.shim_launch_band):
        for n in range(1, 601):
            assert sorted(f(k, n, ways) for k in range(n)) == list(range(n)), (f.__name__, n, ways)


def test_one_way_is_the_identity_and_zero_ways_the_reversal(shim):
    for n in range(1, 601):
        assert [shim.shim_band_of(k, n, 1) for k in range(n)] == list(range(n))
        assert [shim.shim_band_of(k, n, 0) for k in range(n)] == list(range(n - 1, -1, -1))


@pytest.mark.parametrize("ways", [w for w in WAYS if w >= 2])
def test_interleave_deals_distant_segments_in_turn(shim, ways):
    """`ways` contiguous segments of near-equal length, one band of each in turn, every segment walked top to bottom."""
    for n in range(1, 601):
        order = [shim.shim_band_of(k, n, ways) for k in range(n)]
        q, r = divmod(n, ways)
        start = [s * q + min(s, r) for s in range(ways + 1)]                 # segment s = bands [start[s], start[s + 1])
        assert start[ways] == n and all(q <= start[s + 1] - start[s] <= q + 1 for s in range(ways))
        for k in range(q * ways):                                            # whole rounds: round k // ways, segment k % ways
            assert order[k] == start[k % ways] + k // ways, (n, ways, k)
        assert order[q * ways:] == sorted(order[q * ways:])                  # the leftovers: natural order


@pytest.mark.parametrize("ways", WAYS)
def test_small_launches_keep_the_natural_order(shim, ways):
    """Fewer than 2 * ways bands: natural order (the reversal counts as two segments); from there on the map."""
    for n in range(1, 601):
        launch = [shim.shim_launch_band(k, n, ways) for k in range(n)]
        assert launch == (list(range(n)) if n < 2 * max(ways, 2) else [shim.shim_band_of(k, n, ways) for k in range(n)])


@pytest.mark.parametrize("ways", WAYS)
def test_light_rows_are_a_bijection_that_keeps_bands_together(tmp_path, ways):
    s = build_shim(str(tmp_path / ("libdispatchorder_l%d.so" % ways)), ["-DCRY_LIGHT_BAND_WAYS=%d" % ways])
    assert s.shim_light_ways() == ways
    band = s.shim_light_band_rows()
    for rows in range(1, 300):
        got = [s.shim_light_dispatch_row(by, rows) for by in range(rows)]
        assert sorted(got) == list(range(rows)), (rows, ways)
        for by in range(rows // band * band):                                # a band's rows stay consecutive and in order
            assert got[by] % band == by % band and got[by] - got[by - by % band] == by % band
        assert got[rows // band * band:] == list(range(rows // band * band, rows))
        if ways == 1 or rows // band < 2 * max(ways, 2):
            assert got == list(range(rows))


def test_default_ways_are_supported_values(shim):
    assert shim.shim_light_ways() in WAYS and shim.shim_ssao_ways() in WAYS
