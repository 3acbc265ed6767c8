"""The numpy restatement of the pyramid and of step 6b (tests/ssr_gloss_restate.py, from the header alone) against the checker
(tests/ssr_gloss_ref): every byte of the workspace on the pyramid's sizes and on the corpus, and the fetched colour of every hit of the
corpus under the three gloss settings, from the checker's own hit pixel and level word.  All integer: no margins."""
import numpy as np
import pytest

import ssr_gloss_lib as gl
import ssr_gloss_restate as rs
import ssr_lib as sl


@pytest.mark.parametrize("size", gl.PYRAMID_SIZES, ids=lambda s: "%dx%d" % s)
def test_pyramid_restatement_equals_checker(size):
    W, H = size
    img = gl.pyramid_frame(W, H)
    for levels in (8, 4, 1):
        assert np.array_equal(rs.workspace(img, levels, gl.GUARD), gl.pyramid(img, levels)), (size, levels)
        n, sizes, nbytes = gl.plan(W, H, levels)
        assert [s[:2] for s in sizes] == rs.level_sizes(W, H, levels) and ([s[2] for s in sizes], nbytes) == rs.offsets(W, H, levels)


@pytest.mark.parametrize("gname", list(gl.GLOSS_SETS))
def test_fetch_restatement_equals_checker(built_lib, gname):
    hits = blended = 0
    for name, frame, img, pname, _ in sl.corpus():
        pyr, out, n, dbg = gl.expected(name, gname)
        levels = gl.GLOSS_SETS[gname]["levels"]
        assert np.array_equal(rs.workspace(img, levels, gl.GUARD), pyr), name
        ys, xs = np.nonzero(dbg[..., 0] == sl.ST_HIT)
        if not len(ys):
            continue
        hx, hy, lq = (dbg[ys, xs, c].astype(np.int64) for c in (1, 2, 4))
        want = rs.hit_colour(rs.pyramid(img, levels), hx, hy, lq)
        assert np.array_equal(want, dbg[ys, xs, 5:8]), "%s under %s: %d fetched colours differ" % (name, gname, int((want != dbg[ys, xs, 5:8]).any(-1).sum()))
        # at level word 0 the fetch is the point sample
        z = lq == 0
        assert np.array_equal(want[z], img[hy[z], hx[z], :3])
        hits += len(ys)
        blended += int(((lq & 255) > 0).sum())
    assert hits > 1000 and (blended > 100 or gl.GLOSS_SETS[gname]["coneScale"] == 0)
