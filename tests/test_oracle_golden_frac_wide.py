"""The numpy restatements the GPU tests of fhevc_motion_refine_pu_wide compare the kernels with (motion_refine_ref.expected for the 85 nodes,
motion_refine_pu_ref.expected for both PU families) against what the REFERENCE itself returned around integer vectors of up to +-64 samples:
tests/golden/ref_frac_search_wide.npz (TEncSearch::xPatternSearchFracDIF with UseHADME, ranges 24, 33 and 64, windows that reach the replicated
border).  This is also the first time the square refinement above +-8 meets the reference.  No GPU, no oracle/_ref: the golden and the committed
oracle only.  No entry is excluded; the restatements run on the file's five CTUs at each case's own range."""
import numpy as np
import pytest

import motion_golden as mg
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
import motion_refine_wide_cases as wc


@pytest.fixture(scope="module")
def cases():
    return wc.wide_frac_cases()


def long_valid(c, sl):
    """valid entries of the family whose input vector has a component above 8 samples"""
    return (c.out[:, sl, 2] != -1) & (np.abs(c.vin[:, sl].astype(np.int64)).max(axis=-1) > 8)


def test_file_holds_what_the_issue_asks_for(cases):
    assert all((c.W, c.H, c.ctus) == (176, 144, [0, 2, 4, 6, 8]) for c in cases)
    assert {(c.bd, c.R) for c in cases} >= {(8, 64), (8, 33), (10, 64), (12, 24), (12, 64)}
    for c in cases:
        assert 0 <= min(c.cur.min(), c.ref.min()) and max(c.cur.max(), c.ref.max()) < (1 << c.bd)
        assert np.abs(c.vin.astype(np.int64)).max() <= c.R and c.vin.shape == (5, 593, 2) and c.out.shape == (5, 593, 5)
        # the window's own corners in the corner CTUs: (-R, -R) in CTU 0, (R, R) in CTU 8, among valid entries of every family
        for fam, sl in mg.FAMILIES.items():
            valid = c.out[:, sl, 2] != -1
            assert ((c.vin[0, sl] == -c.R).all(axis=-1) & valid[0]).any() and ((c.vin[4, sl] == c.R).all(axis=-1) & valid[4]).any(), (c, fam)
    # the low bits are in use above 8 bit
    assert all((c.cur & ((1 << (c.bd - 8)) - 1)).any() for c in cases if c.bd > 8 and len(np.unique(c.cur)) > 2)
    # the six pan cases of the wide search file on its planes, around its vectors (every 7th entry aside)
    wide = np.load(mg.os.path.join(mg.GOLDEN, "ref_pattern_search_pu_wide.npz"))
    assert len(cases) >= len(wide["cases"]) + 3
    pans = 0
    for k, row in enumerate(wide["cases"]):
        c, p = cases[k], int(row[3])
        assert (c.bd, c.qp, c.R) == tuple(int(v) for v in row[:3]) and np.array_equal(c.cur, wide[f"cur{p}"]) and np.array_equal(c.ref, wide[f"ref{p}"])
        valid = c.out[..., 2] != -1
        assert np.array_equal(valid, wide[f"res{k}"][..., 3] != -1)
        same = (c.vin == wide[f"res{k}"][..., :2]).all(axis=-1)
        keep = np.arange(593) % 7 != 0
        assert same[:, keep][valid[:, keep]].all() and not same[:, ~keep][valid[:, ~keep]].all()
        pans += len(np.unique(c.cur)) > 2
    assert pans == 6
    # long vectors in every family of every case with picture content (the pans and the blended pans), with fractional winners among them
    textured = [c for c in cases if len(np.unique(c.cur)) > 2]
    assert len(textured) >= 8
    for c in textured:
        for fam, sl in mg.FAMILIES.items():
            lv = long_valid(c, sl)
            assert lv.any() and ((c.out[:, sl, 3:5] & 3) != 0).any(axis=-1)[lv].any(), (c, fam)
    # at least one 8-bit case and one above 8 bit (low bits in use) whose winners at long vectors are mostly fractional
    mostly = [c for c in textured if c.R == 33 and all((((c.out[:, sl, 3:5] & 3) != 0).any(axis=-1)[long_valid(c, sl)]).mean() > 0.5 for sl in mg.FAMILIES.values())]
    assert {c.bd for c in mostly} >= {8} and any(c.bd > 8 and (c.cur & ((1 << (c.bd - 8)) - 1)).any() for c in mostly)
    # among the long input vectors every candidate of the half-sample table and of the quarter-sample table wins somewhere; the half stage's winner is
    # not in the file, but the final offset is: 2 h + q with h, q in {-1, 0, 1} reaches all of -3 .. 3 in both directions
    q = np.concatenate([(c.out[..., 3:5] - 4 * c.vin)[long_valid(c, slice(0, 593))] for c in cases])
    assert {tuple(v) for v in q} == {(x, y) for x in range(-3, 4) for y in range(-3, 4)}
    # the swing case: samples 0 and 2^bd - 1 only, 12 bit, random vectors up to +-64
    swing = [c for c in cases if c.bd == 12 and c.R == 64 and set(np.unique(c.ref)) == {0, 4095}]
    assert len(swing) == 1 and np.abs(swing[0].vin.astype(np.int64)).max() == 64


def test_refinement_restatements_equal_the_reference_at_long_vectors(oracle, cases):
    """motion_refine_ref.expected (85 nodes) and motion_refine_pu_ref.expected (both PU families) at each case's R, fed the file's integer vectors: the
    Hadamard distortion at the integer vector, the quarter-sample vector, its distortion and its cost of every valid entry, the marker exactly where
    the file holds -1"""
    done = dict.fromkeys(mg.FAMILIES, 0)
    for c in cases:
        planes = mr.Planes(c.ref, c.bd, c.R + 8)
        got = {"nodes": mr.expected(oracle, np.ascontiguousarray(c.cur).reshape(-1), 0, c.W, c.ref, c.W, c.H, c.bd, c.qp, c.inputs("nodes"), c.R, ctus=c.ctus, planes=planes)}
        for fam in ("pu", "small"):
            got[fam] = rp.expected(oracle, c.cur, c.ref, c.bd, c.qp, c.inputs(fam), c.R, fam, ctus=c.ctus, planes=planes)
        for fam in mg.FAMILIES:
            n = mg.same(got[fam][c.ctus], c.records(fam), (c, fam))
            assert n == wc.PER_CASE[fam]
            done[fam] += n
    assert done == wc.WIDE_FRAC_COUNTS
