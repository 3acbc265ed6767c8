"""crychic_render_sky against its float64 restatement (tests/sky_restate.py: numpy, written from include/crychic_hip.h alone) on the
CPU tier: every channel the restatement decides equals the checker's byte, the marginal ones differ by at most 1 and are few; a table of
misreadings of the definition, each of which the comparison must catch; and the physical known answers of a single-scattering sky, on
the restatement and on the checker's bytes alike."""
import math

import numpy as np
import pytest

import sky_lib as sk
import sky_restate as rs

# Marginal channels -- value * 255 + 0.5 within the restatement's running error bound of an integer, or a texel whose ground, disc or
# planet test lies within its bound of equality -- may be at most this share of the corpus' channels.
MARGINAL_CAP = 0.05
# measured: 0.74 % of the 743 724 channels (most of them the 132 texels of dim 33 whose ray is exactly horizontal in float64 and is
# not in binary32, where (float)33 rcp(33) - 1 is not 0); the largest bound of a channel is 0.04 of a byte


def test_restate_imports_nothing_of_the_code_under_test():
    text = open(rs.__file__).read()
    code = [ln for ln in text.splitlines() if ln.startswith(("import ", "from "))]
    assert code == ["import numpy as np"], code


@pytest.fixture(scope="module")
def restated():
    """{name: (byte, marginal)} over the corpus, computed once."""
    out = {}
    for name, dim, params in sk.corpus():
        out[name] = rs.classify(*rs.restate(dim, params))
    return out


def mismatches(byte, marginal, ref):
    """Channels that break the rule: a decided channel that differs, or a marginal one that differs by more than 1."""
    d = np.abs(byte.astype(np.int32) - ref[..., :3].astype(np.int32))
    return int(((d > 0) & ~marginal).sum() + (d > 1).sum())


def test_decided_channels_equal_the_checker(restated):
    total = marginal = 0
    for name, dim, params in sk.corpus():
        byte, marg = restated[name]
        ref, _ = sk.expected(name)
        assert mismatches(byte, marg, ref) == 0, name
        total += marg.size
        marginal += int(marg.sum())
    share = marginal / total
    print("marginal channels: %d of %d = %.3f %%" % (marginal, total, 100.0 * share))
    assert share <= MARGINAL_CAP, share


@pytest.mark.parametrize("mutation", rs.MUTATIONS)
def test_every_misreading_is_caught(mutation):
    """Each misreading of the definition, restated, breaks the rule on at least one case of the corpus at dim 8, 33 or 64."""
    caught = []
    for name, dim, params in sk.corpus():
        if dim < 8 or dict(sk.DEFAULTS, **params)["viewSteps"] > 16:
            continue
        ref, _ = sk.expected(name)
        n = mismatches(*rs.classify(*rs.restate(dim, params, mutate=mutation)), ref)
        if n:
            caught.append((name, n))
            if len(caught) >= 2:
                break
    assert caught, mutation
    assert len(rs.MUTATIONS) >= 8


# ---- physical known answers, at the defaults, dim 33 --------------------------------------------------------------------------------

DIM = 33


def both(params):
    """[(which, (6, DIM, DIM, 3) bytes)]: the restatement's and the checker's."""
    return [("restatement", rs.classify(*rs.restate(DIM, params))[0]), ("checker", sk.checker(DIM, params)[0][..., :3])]


def luma(t):
    return 77 * int(t[0]) + 150 * int(t[1]) + 29 * int(t[2])


def row_at_elevation(deg):
    """The row of a side face whose centre column looks nearest to `deg` above the horizon, among the rows that look above it: the
    side faces' directions are (.., -t, ..) with t = (2 y + 1) / DIM - 1."""
    el = [math.degrees(math.atan(-((2 * y + 1) / DIM - 1.0))) for y in range(DIM)]
    return min((y for y in range(DIM) if el[y] > 0.0), key=lambda y: abs(el[y] - deg))


def test_a_day_sky_is_blue_and_brighter_near_the_horizon():
    mid = DIM // 2
    for which, cube in both(dict(sunDir=sk.sun_at(30))):        # the sun stands over -z: +Z (face 4) looks away from it
        zenith = cube[2, mid, mid]
        low = cube[4, row_at_elevation(10.0), mid]
        assert zenith[2] > zenith[1] > zenith[0], (which, zenith)
        assert low[2] > low[1] > low[0], (which, low)
        assert luma(low) > luma(zenith), (which, low, zenith)


def test_a_sunset_is_red_towards_the_sun():
    for which, cube in both(dict(sunDir=sk.sun_at(0))):         # -Z (face 5) looks at the sun
        t = cube[5, row_at_elevation(1.0), DIM // 2]
        assert t[0] > t[1] > t[2], (which, t)


def test_night_is_black():
    ref, n = sk.checker(DIM, dict(sunDir=sk.sun_at(-30)))
    assert (ref[..., :3] == 0).all() and (ref[..., 3] == 255).all() and n["black"] == 6 * DIM * DIM
    value, _, _ = rs.restate(DIM, dict(sunDir=sk.sun_at(-30)))
    assert (value == 0.0).all()


def test_a_sun_in_the_plane_x_0_lights_both_sides_alike():
    """Texel (x, y) of +X looks along (1, -t, -s), texel (DIM - 1 - x, y) of -X along (-1, -t, -s): its mirror image."""
    for el in (30, 5):
        for which, cube in both(dict(sunDir=sk.sun_at(el))):
            d = np.abs(cube[0].astype(np.int32) - cube[1][:, ::-1].astype(np.int32))
            assert d.max() <= 1, (which, el, int(d.max()))
