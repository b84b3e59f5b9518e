"""The numpy restatements the GPU tests of config 4 compare the kernels with (motion_pu_ref, motion_pu_small_ref, motion_refine_ref,
motion_refine_pu_ref) against what the REFERENCE itself returned: tests/golden/ref_pattern_search_pu.npz (TEncSearch::xPatternSearch on w x h
patterns, SAD) and tests/golden/ref_frac_search.npz (TEncSearch::xPatternSearchFracDIF with UseHADME around given integer vectors).  Behind the
second file stand the 8-tap filters with their 14-bit intermediate, the rounding of the two-stage path, the order of the half-sample table
against the quarter-sample table, the cost scale of each stage, xGetHADs' choice of 4x4 Hadamards for a side of 4 or 12; behind the first the SAD
of widths 12, 24 and 48 and the raster order of ties.  No GPU, no oracle/_ref: goldens and the committed oracle only.  No entry is excluded."""
import numpy as np
import pytest

import motion_golden as mg
import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_refine_pu_ref as rp
import motion_refine_ref as mr


@pytest.fixture(scope="module")
def search_cases():
    return mg.search_cases()


@pytest.fixture(scope="module")
def frac_cases():
    return mg.frac_cases()


def test_files_hold_what_the_issue_asks_for(search_cases, frac_cases):
    for cases in (search_cases, frac_cases):
        assert {c.bd for c in cases} == {8, 10, 12} and {0, 32, 51} <= {c.qp for c in cases} and {1, 5, 8} <= {c.R for c in cases}
        assert all((c.W, c.H, c.ctus) == (176, 144, [0, 2, 4, 6, 8]) for c in cases)
        for c in cases:   # the low bits are in use above 8 bit, and no sample leaves the bit depth
            assert 0 <= min(c.cur.min(), c.ref.min()) and max(c.cur.max(), c.ref.max()) < (1 << c.bd)
        assert any(c.bd > 8 and (c.cur & ((1 << (c.bd - 8)) - 1)).any() for c in cases)
    # widths 12, 24 and 48 are among the searched PUs, and blocks with a side of 4 or 12 among the refined ones
    widths = {mp.pu_rect(*e)[2] for e in mp.covered()} | {mp.pu_rect(*e)[2] for e in ps.covered()}
    assert {4, 8, 12, 16, 24, 32, 48, 64} <= widths
    # the winners leave the integer grid in every direction, as far as the two stages reach (the generator itself asserts that each of the nine
    # candidates of either stage wins somewhere); corner vectors reach the replicated border
    q = np.concatenate([(c.out[..., 3:5] - 4 * c.vin)[c.out[..., 2] != -1] for c in frac_cases])
    assert {tuple(v) for v in q} >= {(x, y) for x in (-3, 0, 3) for y in (-3, 0, 3)} and np.abs(q).max() == 3 and (q != 0).any(axis=1).mean() > 0.2
    assert any((c.vin[0] == -c.R).all(axis=-1).any() for c in frac_cases) and any((c.vin[4] == c.R).all(axis=-1).any() for c in frac_cases)


def test_search_restatements_equal_the_reference(oracle, search_cases):
    """motion_pu_ref.expected (85 nodes, 124 PUs) and motion_pu_small_ref.expected (384 small PUs) in SAD mode: vector, SAD, cost and the SAD at
    the zero vector of every valid entry, the marker exactly where the file holds -1"""
    done = dict.fromkeys(mg.FAMILIES, 0)
    for c in search_cases:
        nodes, pus = mp.expected(oracle, c.cur, c.ref, c.bd, c.qp, c.R, True, ctus=c.ctus)
        small = ps.expected(oracle, c.cur, c.ref, c.bd, c.qp, c.R, True, ctus=c.ctus)
        for fam, got in (("nodes", nodes), ("pu", pus), ("small", small)):
            done[fam] += mg.same(got[c.ctus].astype(mg.capi.MOTION_DTYPE), c.records(fam), (c, fam))
    assert done == mg.SEARCH_COUNTS


def test_refinement_restatements_equal_the_reference(oracle, frac_cases):
    """motion_refine_ref.expected (85 nodes) and motion_refine_pu_ref.expected (both PU families) fed the file's integer vectors: the Hadamard
    distortion at the integer vector, the quarter-sample vector, its distortion and its cost"""
    done = dict.fromkeys(mg.FAMILIES, 0)
    for c in frac_cases:
        planes = mr.Planes(c.ref, c.bd, 16)
        got = {"nodes": mr.expected(oracle, np.ascontiguousarray(c.cur).reshape(-1), 0, c.W, c.ref, c.W, c.H, c.bd, c.qp, c.inputs("nodes"), c.R, ctus=c.ctus, planes=planes)}
        for fam in ("pu", "small"):
            got[fam] = rp.expected(oracle, c.cur, c.ref, c.bd, c.qp, c.inputs(fam), c.R, fam, ctus=c.ctus, planes=planes)
        for fam in mg.FAMILIES:
            done[fam] += mg.same(got[fam][c.ctus], c.records(fam), (c, fam))
    assert done == mg.FRAC_COUNTS
