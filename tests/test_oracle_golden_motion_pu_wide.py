"""The numpy restatements the GPU tests of fhevc_motion_search_pu_wide compare the kernels with (motion_pu_ref.expected, motion_pu_small_ref.expected
in SAD mode) against what the REFERENCE itself returned at HM's own SearchRange: tests/golden/ref_pattern_search_pu_wide.npz
(TEncSearch::xPatternSearch on w x h patterns, ranges 24, 33 and 64, where every window of the 176 x 144 picture reaches the replicated border).
No GPU, no oracle/_ref: the golden and the committed oracle only.  No entry is excluded; the restatements run on the file's five CTUs."""
import numpy as np
import pytest

import motion_golden as mg
import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_pu_wide_cases as wc


@pytest.fixture(scope="module")
def cases():
    return wc.wide_cases()


def test_file_holds_what_the_issue_asks_for(cases):
    assert all((c.W, c.H, c.ctus) == (176, 144, [0, 2, 4, 6, 8]) for c in cases)
    assert {(c.bd, c.R) for c in cases} >= {(8, 64), (8, 33), (10, 64), (12, 24)}
    for c in cases:
        assert 0 <= min(c.cur.min(), c.ref.min()) and max(c.cur.max(), c.ref.max()) < (1 << c.bd)
    # the low bits are in use above 8 bit
    assert all((c.cur & ((1 << (c.bd - 8)) - 1)).any() for c in cases if c.bd > 8)
    # 8 bit at both ranges on two different clips; long vectors in every family of every pan case
    pans = [c for c in cases if len(np.unique(c.cur)) > 2]
    assert len({c.cur.tobytes() for c in pans if c.bd == 8}) == 2 and len([c for c in pans if c.bd == 8]) >= 4
    for c in pans:
        for fam, sl in mg.FAMILIES.items():
            r = c.res[:, sl]
            assert np.abs(r[..., :2][r[..., 3] != -1]).max() > 8, (c, fam)
    # the two contents whose ties raster order decides, at R = 64
    flat = [c for c in cases if len(np.unique(c.cur)) <= 2]
    assert len(flat) == 2 and all(c.R == 64 for c in flat)
    white = next(c for c in flat if len(np.unique(c.cur)) == 1)
    r = white.res[white.res[..., 3] != -1]
    assert (r[:, :2] == 0).all()          # every vector has the same SAD: the cheapest vector cost wins, the zero vector


def test_search_restatements_equal_the_reference(oracle, cases):
    """vector, SAD, cost and the SAD at the zero vector of every valid entry, the marker exactly where the file holds -1"""
    done = dict.fromkeys(mg.FAMILIES, 0)
    for c in cases:
        nodes, pus = mp.expected(oracle, c.cur, c.ref, c.bd, c.qp, c.R, True, ctus=c.ctus)
        small = ps.expected(oracle, c.cur, c.ref, c.bd, c.qp, c.R, True, ctus=c.ctus)
        for fam, got in (("nodes", nodes), ("pu", pus), ("small", small)):
            n = mg.same(got[c.ctus].astype(mg.capi.MOTION_DTYPE), c.records(fam), (c, fam))
            assert n == wc.PER_CASE[fam]
            done[fam] += n
    assert done == wc.WIDE_COUNTS
