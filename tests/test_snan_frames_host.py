"""Signaling NaNs in whole frames, CPU tier: the kernel bodies compiled for the host over tests/snan_frames.py's planes against the
oracle and the features' checkers.  Bar: test_fuzz.py's -- AO and RGBA8 bit-exact, radiance equal up to NaN payloads.  The device twin
is tests/test_snan_frames_gpu.py."""
import numpy as np
import pytest

import snan_frames
from fuzz_util import same_floats


def frames_equal(got, ref):
    return np.array_equal(got[0], ref[0]) and same_floats(got[1], ref[1])


@pytest.mark.parametrize("size", snan_frames.SIZES)
def test_signaling_nans_in_the_planes_kernel_bodies(built_lib, oracle, hostsim, size):
    import env_brdf_lib
    r = snan_frames.reference(size, built_lib)
    W, H, p, c, knobs = r["W"], r["H"], r["planes"], r["c"], r["knobs"]
    for k, n in (("normal", 16), ("g0", 32), ("g1", 32), ("g2", 32)):       # the planes hold what the test is about
        u = p[k].view(np.uint16 if n == 16 else np.uint32)
        pats = snan_frames.HALF_PATTERNS if n == 16 else snan_frames.FLOAT_PATTERNS
        share = np.isin(u, pats).any(-1).mean()
        assert all((u == v).any() for v in pats) and 0.01 < share < 0.03, (k, share)
    assert r["bite"] >= 1, "no pixel whose only NaN input is signaling has a finite radiance: the frame cannot tell"
    ndl, radius, sky = knobs["numDirLights"], knobs["pcfSearchRadius"], knobs["sky"]
    ao, _ = hostsim.compute_ssao(c.ssao_cb, p["normal"], p["depth"], p["randvec"], int(built_lib.lib.crychic_edge_plane_bytes(W, H)), 2)
    assert np.array_equal(ao, r["ao"]), size
    got = hostsim.light(c.pass_cb, p["g0"], p["g1"], p["g2"], p["depth"], r["ao"], p["shadow"], p["cube"], ndl, radius, flags=sky, want_radiance=True)
    assert frames_equal(got, r["plain"]), ("plain", size)
    only = snan_frames.only_signaling(p)
    assert np.array_equal(got[0][only], r["plain"][0][only]) and same_floats(got[1][only], r["plain"][1][only])
    got = hostsim.light(c.pass_cb, p["g0"], p["g1"], p["g2"], p["depth"], r["ao"], p["shadow"], r["chain_cube"], ndl, radius, flags=sky,
                        want_radiance=True, **r["chain_kw"])
    assert frames_equal(got, r["chain"]), ("derivative chain", size)
    got = env_brdf_lib.load().host_light(c.pass_cb, r["spec_planes"], None, ndl, radius, r["spec_flags"], cube_dim=r["chain_kw"]["cube_dim"])
    assert frames_equal(got, r["spec"]), ("gloss + SH + split-sum", size)
    h = r["half_planes"]
    got = hostsim.light(c.pass_cb, h["g0"], h["g1"], h["g2"], h["depth"], r["ao"], h["shadow"], h["cube"], ndl, radius, flags=sky, want_radiance=True)
    assert frames_equal(got, r["half"]), ("all-half mix", size)
