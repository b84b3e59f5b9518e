"""tests/motion_range_sweep.py -- the expected records of the integer motion searches at every range from one +-64 SAD volume -- pinned before
any kernel is held to it (tests/test_gpu_motion_range_sweep.py): against the per-range restatements (motion_pu_ref.expected,
motion_pu_small_ref.expected) on the sweep clips, against what the REFERENCE itself returned (tests/golden/ref_pattern_search_pu_wide.npz at
ranges 24, 33 and 64, tests/golden/ref_pattern_search_pu.npz at 1, 5 and 8), and the conditions on the clips' content that give the sweep its
teeth: at every range winners sit on all four edges of the window, where the kernels hold their last block of dy and their last group of dx, and
strictly inside it.  No GPU, no oracle/_ref: the committed oracle and goldens only."""
import numpy as np
import pytest

import motion_golden as mg
import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_pu_wide_cases as wc
import motion_range_sweep as sw

BDS = (8, 10, 12)
EDGES = ("mvy=-R", "mvy=+R", "mvx=-R", "mvx=+R")


def restated(oracle, cur, ref, bd, qp, R, sad, ctus=None):
    nodes, pus = mp.expected(oracle, cur, ref, bd, qp, R, sad, ctus=ctus)
    return {"nodes": nodes, "pu": pus, "small": ps.expected(oracle, cur, ref, bd, qp, R, sad, ctus=ctus)}


def same_records(got, exp, what):
    """every field of every entry, markers included -> the number of valid entries compared"""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    for k in sw.DT.names:
        bad = got[k] != exp[k]
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[k][bad][:5].tolist(), exp[k][bad][:5].tolist())
    return int((exp["cost_best"] != sw.MARKER).sum())


# ---- 1. the per-range restatements ----------------------------------------------------------------------------------------------------------------------

def test_geometry_of_the_sweep_picture():
    """104 x 88: one whole CTU, one 40 wide, one 24 tall, the corner; the valid entries counted by hand"""
    assert (sw.W, sw.H, sw.NF) == (104, 88, 3)
    # CTU 1 (40 x 64): 2 32x32, 8 16x16, 40 8x8 nodes; CTU 2 (64 x 24): 4 16x16, 24 8x8; CTU 3 (40 x 24): 2 16x16, 15 8x8
    assert sw.valid_counts() == {"nodes": 85 + 50 + 28 + 17, "pu": 124 + (2 * 12 + 8 * 4) + 4 * 4 + 2 * 4,
                                 "small": 384 + (8 * 8 + 40 * 4) + (4 * 8 + 24 * 4) + (2 * 8 + 15 * 4)}
    for name in sw.CLIPS:
        pics = sw.clip(name)
        assert len(pics) == 3 and all(p.shape == (88, 104) and p.dtype == np.uint8 for p in pics)
        for bd in (10, 12):
            assert all((p & ((1 << (bd - 8)) - 1)).any() and p.max() < (1 << bd) for p in sw.planes(name, bd))


@pytest.mark.parametrize("sad", [True, False], ids=["sad", "satd"])
@pytest.mark.parametrize("bd", BDS)
def test_small_ranges_equal_the_restatements(oracle, bd, sad):
    """ranges 1, 4, 7 and 8 of every clip, both picture pairs, all four CTUs: the sub-window of the +-64 SAD volume, and the sub-window of the +-8
    Hadamard distortions"""
    counts = sw.valid_counts()
    for name in sw.CLIPS:
        p, qp = sw.planes(name, bd), sw.clip_qp(name, bd)
        for pair, s in enumerate(sw.sweep(oracle, name, bd, sad)):
            for R in (1, 4, 7, 8):
                exp = restated(oracle, p[pair + 1], p[pair], bd, qp, R, sad)
                got = s.records(R)
                for f in sw.FAMS:
                    assert same_records(got[f], exp[f].astype(sw.DT), (name, bd, sad, pair, R, f)) == counts[f]


@pytest.mark.parametrize("name,bd", [("diag", 8), ("anti", 10), ("slow", 12)])
def test_ranges_12_and_33_equal_the_restatements(oracle, name, bd):
    """the whole CTU of the first pair and the three ragged ones of the second"""
    p, qp = sw.planes(name, bd), sw.clip_qp(name, bd)
    for pair, ctus in ((0, [0]), (1, [1, 2, 3])):
        s = sw.sweep(oracle, name, bd)[pair]
        for R in (12, 33):
            exp = restated(oracle, p[pair + 1], p[pair], bd, qp, R, True, ctus=ctus)
            got = s.records(R)
            for f in sw.FAMS:
                n = same_records(got[f][ctus], exp[f][ctus].astype(sw.DT), (name, bd, pair, R, f))
                assert n == int(s.valid[f][ctus].sum()) > 0


# ---- 2. what the reference itself returned --------------------------------------------------------------------------------------------------------------

def golden_sweeps(oracle, cases, rmax):
    """one PairSweep per distinct (pictures, bit depth) of a golden file, at the QPs of all its cases"""
    groups = {}
    for c in cases:
        groups.setdefault((c.cur.tobytes(), c.ref.tobytes(), c.bd), []).append(c)
    out = {}
    for g in groups.values():
        s = sw.PairSweep(oracle, g[0].cur, g[0].ref, g[0].bd, g[0].qp, ctus=g[0].ctus, rmax=rmax, more_qps=[c.qp for c in g])
        for c in g:
            out[c.k] = s
    return out


@pytest.mark.parametrize("which", ["wide", "small"])
def test_sweep_equals_the_reference(oracle, which):
    """every valid entry of all three families of the files' five CTUs; the marker exactly where the file holds -1"""
    cases, total, rmax = (wc.wide_cases(), wc.WIDE_COUNTS, 64) if which == "wide" else (mg.search_cases(), mg.SEARCH_COUNTS, 8)
    assert {c.R for c in cases} >= ({24, 33, 64} if which == "wide" else {1, 5, 8})
    sweeps = golden_sweeps(oracle, cases, rmax)
    done = dict.fromkeys(sw.FAMS, 0)
    for c in cases:
        got = sweeps[c.k].at(c.qp, c.R)
        for f in sw.FAMS:
            done[f] += mg.same(got[f][c.ctus], c.records(f), (c, f))
    assert done == total


# ---- 3. the content of the clips ------------------------------------------------------------------------------------------------------------------------

def edge_counts(s, R, fams=sw.FAMS):
    """[mvy = -R, mvy = +R, mvx = -R, mvx = +R, strictly inside] among the valid entries of a clip's two pairs"""
    cnt = np.zeros(5, np.int64)
    for pair in s:
        for f in fams:
            r = pair.rec[f][R][pair.valid[f]]
            x, y = r["mvx"].astype(np.int64), r["mvy"].astype(np.int64)
            cnt += [(y == -R).sum(), (y == R).sum(), (x == -R).sum(), (x == R).sum(), ((np.abs(x) < R) & (np.abs(y) < R)).sum()]
    return cnt


@pytest.mark.parametrize("bd", BDS)
def test_winners_on_every_edge_and_inside_at_every_range(oracle, bd):
    """the last dy block (moved up to range - (DB - 1)), the last dx group (masked past +R) and the first chunk of the window (dropped or split
    at column 0) hold the vectors on the window's edges: a kernel that loses one of them loses a winner here"""
    per_family = {f: np.zeros(4, np.int64) for f in sw.FAMS}
    for name in sw.CLIPS:
        s = sw.sweep(oracle, name, bd)
        for R in range(1, 65):
            cnt = edge_counts(s, R)
            assert cnt.min() >= 8, (name, bd, R, dict(zip(EDGES + ("inside",), cnt.tolist())))
            for f in sw.FAMS:
                per_family[f] += edge_counts(s, R, (f,))[:4] > 0
    # over the sweep each family has winners on every edge -- at most of the ranges, in fact
    for f in sw.FAMS:
        assert (per_family[f] >= 3 * 48).all(), (bd, f, per_family[f].tolist())


def test_first_window_columns_hold_winners_where_the_dword_branch_drops_a_dword(oracle):
    """delta = 4 (R = 12, 20, .., 60): the window's first chunk starts at column -4, its low dword is dropped and its high dword is window columns
    0..3.  Entries of the CTU's first column win at mvx = -R there, so those four columns decide records"""
    for R in range(12, 64, 8):
        n = 0
        for name in sw.CLIPS:
            for pair in sw.sweep(oracle, name, 8):
                for f in sw.FAMS:
                    x0 = np.array([e[1] for e in sw.ENTRIES[f]])
                    r = pair.rec[f][R]
                    n += int((pair.valid[f] & (x0[None, :] + r["mvx"].astype(np.int64) + R <= 3)).sum())
        assert n >= 8, (R, n)


def test_ties_go_to_the_raster_first_vector_of_least_cost(oracle):
    """a flat pair: every vector has the same SAD, so the vector cost alone decides, and among equal costs the raster order"""
    flat = np.full((sw.H, sw.W), 100, np.int64)
    qp = 30
    s = sw.PairSweep(oracle, flat + 3, flat, 8, qp)
    costs = sw.cost_window(oracle, 64, mp.sqrt_lambda(oracle, qp, 8))
    for R in range(1, 65):
        sub = costs[64 - R:64 + R + 1, 64 - R:64 + R + 1]
        m = int(np.argmin(sub))          # the first minimum in raster order
        for f in sw.FAMS:
            r = s.rec[f][R][s.valid[f]]
            area = np.array([e[3] * e[4] for e in sw.ENTRIES[f]])
            exp_sad = np.broadcast_to(3 * area, s.valid[f].shape)[s.valid[f]]
            assert (r["mvx"] == m % (2 * R + 1) - R).all() and (r["mvy"] == m // (2 * R + 1) - R).all(), (R, f)
            assert np.array_equal(r["satd_best"], exp_sad) and np.array_equal(r["satd_zero"], exp_sad) and np.array_equal(r["cost_best"], exp_sad + sub.reshape(-1)[m])
    # ... and where the cost does not decide either: two vectors of equal cost and equal SAD, the earlier row wins, then the earlier column
    E = np.full((1, 5, 5), 7, np.int32)
    c = np.full((5, 5), 9, np.int64)
    c[1, 3] = c[3, 1] = c[1, 1] = 2
    w = sw.winners(E, c)
    assert (int(w[1, 0]["mvx"]), int(w[1, 0]["mvy"])) == (-1, -1) and (int(w[2, 0]["mvx"]), int(w[2, 0]["mvy"])) == (-1, -1) and w[2, 0]["cost_best"] == 9
    c[1, 1] = 9
    w = sw.winners(E, c)
    assert (int(w[1, 0]["mvx"]), int(w[1, 0]["mvy"])) == (1, -1) and w[0, 0]["cost_best"] == 16
