"""tests/p_tree_ref.py (the Python restatement of the tree decision) against hand-computed CTUs: a handful of costs set by hand.  No GPU.  The last
tests confirm, on the CPU restatements of the searches, refinements and the selection, the map that tests/test_gpu_p_tree.py expects of the real chains."""
import itertools

import numpy as np
import pytest

import p_tree_ref as tr
from fasthevc_amd import capi

M, SAT = tr.MARK, tr.SAT
S, T, X, A, O, K = tr.SPLIT_SURE, tr.STOP_SURE, tr.CROSSING, tr.ABSENT, tr.OWN_AVAILABLE, tr.KIDS_AVAILABLE


def flat(leaf=10):
    """a whole CTU in which nothing splits: every leaf costs `leaf`, every node above one less than its four children together"""
    c = np.zeros(85, np.uint32)
    c[21:] = leaf
    c[5:21] = 4 * leaf - 1
    c[1:5] = 4 * (4 * leaf - 1) - 1
    c[0] = 4 * (4 * (4 * leaf - 1) - 1) - 1
    return c


def fields(rec, k):
    return int(rec["cost_own"][k]), int(rec["cost_kids"][k]), int(rec["cost_tree"][k]), int(rec["flags"][k])


def test_a_whole_ctu_by_hand():
    c = flat()
    rec, dmin, dmax = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 84) == (10, M, 10, O) and rec["level"][84] == 3 and (rec["pad"] == 0).all()
    assert fields(rec, 5) == (39, 40, 39, T | O | K)
    assert fields(rec, 1) == (155, 156, 155, T | O | K)
    assert fields(rec, 0) == (619, 620, 619, T | O | K)
    assert rec["level"].tolist() == [0] + [1] * 4 + [2] * 16 + [3] * 64
    assert (dmin == 0).all() and (dmax == 0).all()
    # one 16x16 (node 10: nx 1, ny 1) whose leaves add up to 35: it splits, and the 4 it saves make its 32x32 and the CTU split as well
    c[21 + 2 * 8 + 2] = c[21 + 2 * 8 + 3] = c[21 + 3 * 8 + 2] = 9
    c[21 + 3 * 8 + 3] = 8
    rec, dmin, dmax = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 10) == (39, 35, 35, S | O | K)
    assert fields(rec, 1) == (155, 152, 152, S | O | K)          # 35 + 3 * 39 = 152 < 155
    assert fields(rec, 0) == (619, 617, 617, S | O | K)          # 152 + 3 * 155 = 617 < 619
    exp = np.zeros((16, 16), np.uint8)
    exp[0:8, 0:8] = 2
    exp[4:8, 4:8] = 3
    exp[0:8, 8:16] = 1
    exp[8:16, :] = 1
    assert np.array_equal(dmin.reshape(16, 16), exp) and np.array_equal(dmax, dmin)


def test_tie_does_not_split_and_one_less_does():
    c = flat()
    c[5] = 40                                    # kids == own
    rec, dmin, dmax = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 5) == (40, 40, 40, T | O | K)
    c[5] = 41                                    # kids == own - 1
    rec, _, _ = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 5) == (41, 40, 40, S | O | K)


def only_root(own, leaf_sum_quarter):
    """a CTU in which only the root's decision is open: its four children cost leaf_sum_quarter each and never split"""
    c = np.zeros(85, np.uint32)
    c[21:] = 0xFFFFFFF0
    c[5:21] = 0xFFFFFFF0
    c[1:5] = leaf_sum_quarter
    c[0] = own
    return c


@pytest.mark.parametrize("lvl", [0, 1, 2])
def test_margins_on_either_side_of_each_inequality(lvl):
    """own 1000, kids 4 * 200 = 800 at one node of level lvl (everything else cannot split)"""
    k = (0, 2, 9)[lvl]
    c = np.full(85, 0x10000000, np.uint32)
    c[21:] = 0x10000000
    for ch in tr.children(k):
        c[ch] = 200
        if lvl < 2:
            for g in tr.children(ch):
                c[g] = 0x10000000        # the children themselves never split
    c[k] = 1000
    three = lambda v: [v if l == lvl else 0 for l in range(3)]
    flags = lambda **kw: fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(**{n: three(v) for n, v in kw.items()}))[0], k)
    assert flags() == (1000, 800, 800, S | O | K)
    # split_sure: 800 + abs < 1000
    assert flags(split_abs=199)[3] == S | O | K and flags(split_abs=200)[3] == O | K
    # 800 + (800 * q8 >> 8) < 1000: q8 = 63 -> 196, q8 = 64 -> 200
    assert flags(split_q8=63)[3] == S | O | K and flags(split_q8=64)[3] == O | K
    assert flags(split_q8=65535)[3] == O | K
    # margins never enter tree
    assert flags(split_q8=65535, split_abs=0x7FFFFFFF)[:3] == (1000, 800, 800)
    # the margin is per level
    other = [0x7FFFFFFF if l != lvl else 0 for l in range(3)]
    assert fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(split_abs=other))[0], k)[3] == S | O | K
    # stop_sure: own + abs + (own * q8 >> 8) <= kids, with own 700: 700 + 100 <= 800, 700 + 101 > 800
    c[k] = 700
    assert flags() == (700, 800, 700, T | O | K)
    assert flags(stop_abs=100)[3] == T | O | K and flags(stop_abs=101)[3] == O | K
    # 700 * 36 >> 8 = 98, 700 * 37 >> 8 = 101
    assert flags(stop_q8=36)[3] == T | O | K and flags(stop_q8=37)[3] == O | K
    assert flags(stop_q8=65535)[3] == O | K
    # "neither" leaves depth_min above the node and depth_max below it
    _, dmin, dmax = tr.tree_ctu(c, 64, 64, capi.p_tree_rule(stop_abs=three(101)))
    l, nx, ny = tr.node_pos(k)
    u = 16 >> l
    inside = (slice(ny * u, ny * u + u), slice(nx * u, nx * u + u))
    assert (dmax.reshape(16, 16)[inside] >= dmin.reshape(16, 16)[inside]).all()
    if lvl == 0:
        assert (dmin == 0).all() and (dmax == 1).all()


def test_costs_near_2_32_do_not_wrap():
    # own 0xFFFFFFFD against kids 4 * 0x3FFFFFFF = 0xFFFFFFFC: splits by one; with split_abs 1 it no longer does.  kids * q8 at q8 = 65535 is about 2^48:
    # in 32 bits the limit would wrap below own and the node would split
    c = only_root(0xFFFFFFFD, 0x3FFFFFFF)
    rec, _, _ = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 0) == (0xFFFFFFFD, 0xFFFFFFFC, 0xFFFFFFFC, S | O | K)
    assert fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(split_abs=1))[0], 0)[3] == O | K
    assert fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(split_q8=65535))[0], 0)[3] == O | K
    # stop side: own 0xFFFFFFFC, kids SAT (a saturated sum): own + 2 <= SAT, own + 3 is not; own * q8 and own + 0x7FFFFFFF would wrap in 32 bits and stop
    c = only_root(0xFFFFFFFC, 0x7FFFFFFF)
    rec, _, _ = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 0) == (0xFFFFFFFC, SAT, 0xFFFFFFFC, T | O | K)
    assert fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(stop_abs=2))[0], 0)[3] == T | O | K
    assert fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(stop_abs=3))[0], 0)[3] == O | K
    assert fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(stop_q8=65535))[0], 0)[3] == O | K
    assert fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(stop_q8=1, stop_abs=0x7FFFFFFF))[0], 0)[3] == O | K


def test_saturation():
    c = only_root(M - 2, 0x7FFFFFFF)              # 4 * 0x7FFFFFFF = 0x1FFFFFFFC -> SAT
    rec, _, _ = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 0) == (M - 2, SAT, M - 2, T | O | K)
    # a saturated sum is available and is not the marker: a parent whose own cost is the marker takes it
    c[0] = M
    rec, _, _ = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 0) == (M, SAT, SAT, K)
    # split_cost saturates as well
    c = only_root(5000, 1000)
    rec, _, _ = tr.tree_ctu(c, 64, 64, capi.p_tree_rule(split_cost=[0x7FFFFFFF, 0, 0]))
    assert fields(rec, 0) == (5000, 4000 + 0x7FFFFFFF, 5000, T | O | K)
    c = only_root(5000, 0x3FFFFFFF)
    rec, _, _ = tr.tree_ctu(c, 64, 64, capi.p_tree_rule(split_cost=[3, 0, 0]))
    assert fields(rec, 0)[1] == SAT
    rec, _, _ = tr.tree_ctu(c, 64, 64, capi.p_tree_rule(split_cost=[2, 0, 0]))
    assert fields(rec, 0)[1] == SAT and 4 * 0x3FFFFFFF + 2 == SAT


def test_marks():
    c = flat()
    # own MARK with kids available: the tree is the children's, no decision, depth_min stays above, depth_max goes below
    c[0] = M
    rec, dmin, dmax = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 0) == (M, 620, 620, K)
    assert (dmin == 0).all() and (dmax == 1).all()
    # kids MARK with own available: one marked leaf marks the children's sum of its 16x16 only -- that node falls back on its own cost
    c = flat()
    c[21] = M
    rec, dmin, dmax = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 21) == (M, M, M, 0)
    assert fields(rec, 5) == (39, M, 39, O)
    assert fields(rec, 1) == (155, 156, 155, T | O | K)
    assert (dmin == 0).all() and (dmax == 0).all()
    # both MARK gives MARK, and that travels up through every node whose own cost is the marker as well
    c[5] = M
    rec, dmin, dmax = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 5) == (M, M, M, 0)
    assert fields(rec, 1) == (155, M, 155, O)
    c[1] = M
    c[0] = M
    rec, dmin, dmax = tr.tree_ctu(c, 64, 64)
    assert fields(rec, 1) == (M, M, M, 0) and fields(rec, 0) == (M, M, M, 0)
    assert (dmin == 0).all()
    assert (dmax.reshape(16, 16)[:4, :4] == 3).all() and (dmax.reshape(16, 16)[8:, 8:] == 1).all()


def test_mark_travels_up_a_crossing_chain_to_the_root():
    """valid 40 x 40: the root, the 32x32 nodes 2, 3, 4 and the 16x16 nodes along the edge cross; a marked leaf under them reaches the root"""
    c = flat()
    rec, dmin, dmax = tr.tree_ctu(c, 40, 40)
    assert fields(rec, 0)[3] == X | K and fields(rec, 2)[3] == X | K and fields(rec, 1)[3] == T | O | K
    # node 2 (x 32..63): its 16x16 children 7 (32..47: crossing, leaves at x = 32 inside) and 11; 8 and 12 are outside
    assert fields(rec, 7) == (M, 20, 20, X | K) and fields(rec, 8) == (M, M, M, A) and fields(rec, 11) == (M, 20, 20, X | K)
    assert fields(rec, 2) == (M, 40, 40, X | K)
    # the root: node 1 (155) + node 2 (40) + node 3 (40) + node 4 (one leaf: 10), no split cost on crossing nodes
    assert fields(rec, 4) == (M, 10, 10, X | K) and fields(rec, 0) == (M, 245, 245, X | K)
    rec5, _, _ = tr.tree_ctu(c, 40, 40, capi.p_tree_rule(split_cost=[1000, 100, 10]))
    assert fields(rec5, 0) == (M, 245, 245, X | K) and fields(rec5, 1) == (155, 156 + 100, 155, T | O | K)
    leaf = 21 + 4 * 8 + 4                         # the 8x8 at (32, 32): the one coded leaf of node 4
    assert fields(rec, leaf) == (10, M, 10, O) and fields(rec, leaf + 1) == (M, M, M, A)
    c[leaf] = M
    rec, dmin, dmax = tr.tree_ctu(c, 40, 40)
    assert fields(rec, 15)[3] == X                         # node 15 = the 16x16 at (32, 32)
    assert fields(rec, 4) == (M, M, M, X) and fields(rec, 0) == (M, M, M, X)
    m = dmin.reshape(16, 16)
    assert (m[:, 10:] == 0).all() and (m[10:, :] == 0).all() and (m[:8, :8] == 1).all() and (m[8:10, 8:10] == 3).all() and np.array_equal(dmin, dmax)


def test_split_cost_is_added_for_inside_nodes_only():
    c = flat()
    c[5] = 45                                     # kids 40 < own 45: splits; with a split cost of 5 it ties and no longer does
    r = lambda sc: fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(split_cost=[0, 0, sc]))[0], 5)
    assert r(0) == (45, 40, 40, S | O | K) and r(4) == (45, 44, 44, S | O | K) and r(5) == (45, 45, 45, T | O | K)
    # levels are separate
    assert fields(tr.tree_ctu(c, 64, 64, capi.p_tree_rule(split_cost=[7, 7, 0]))[0], 5) == (45, 40, 40, S | O | K)


@pytest.mark.parametrize("vw,vh", list(itertools.product((8, 12, 36, 40, 64), repeat=2)))
def test_every_geometry(vw, vh):
    rng = np.random.default_rng(vw * 100 + vh)
    c = rng.integers(1, 1000, size=85).astype(np.uint32)
    rec, dmin, dmax = tr.tree_ctu(c, vw, vh, tr.random_rule(rng))
    m, x = dmin.reshape(16, 16), dmax.reshape(16, 16)
    uw, uh = (vw + 3) // 4, (vh + 3) // 4
    assert (m[:, uw:] == 0).all() and (m[uh:, :] == 0).all() and (x[:, uw:] == 0).all() and (x[uh:, :] == 0).all()
    assert (m <= x).all()
    for k in range(85):
        l, nx, ny = tr.node_pos(k)
        s = 64 >> l
        inside = nx * s + s <= vw and ny * s + s <= vh
        outside = nx * s >= vw or ny * s >= vh
        f = int(rec["flags"][k])
        if outside or (l == 3 and not inside):
            assert fields(rec, k) == (M, M, M, A), k
        elif inside:
            assert not f & (X | A) and f & O and rec["cost_own"][k] == c[k], k
        else:
            assert f & X and not f & (A | O | S | T) and rec["cost_own"][k] == M and rec["cost_tree"][k] == rec["cost_kids"][k], k
    # units under a crossing node are at least one level below it
    if vw < 64 or vh < 64:
        assert (m[:uh, :uw] >= 1).all()
    if vw == 64 and vh == 64:
        assert not (rec["flags"] & (X | A)).any()


def test_properties_on_random_draws():
    rng = np.random.default_rng(4)
    shapes = tr.random_shapes(rng, 3, 12)
    for i in range(8):
        rule = tr.random_rule(rng)
        for W, H in ((200, 136), (100, 76)):
            n = ((W + 63) // 64) * ((H + 63) // 64)
            rec, dmin, dmax = tr.select(shapes[:, :n], W, H, rule=rule)
            assert (dmin <= dmax).all()
            assert not ((rec["flags"] & S != 0) & (rec["flags"] & T != 0)).any()
            drec, lo, hi = tr.select(shapes[:, :n], W, H)
            # the default rule decides every node that has both costs one way or the other
            both = (drec["flags"] & (O | K)) == (O | K)
            assert (((drec["flags"][both] & S) != 0) != ((drec["flags"][both] & T) != 0)).all()
            # ... so the maps differ only under nodes where a marker is involved
            for p, c in zip(*np.nonzero((lo != hi).any(axis=2))):
                f = drec["flags"][p, c, :21]
                assert ((f & (X | A)) == 0)[(f & (O | K)) != (O | K)].any(), (p, c)
    clean = shapes.copy()
    clean["cost_best"][clean["cost_best"] == M] = 77
    _, lo, hi = tr.select(clean[:, :12], 200, 136)
    assert np.array_equal(lo, hi)


# ---- the constructed pairs, confirmed on the CPU restatements -----------------------------------------------------------------------------------------

def test_constructed_motions_give_the_expected_map(oracle):
    import p_tree_cases as tc
    case = tc.constructed_case(oracle)
    tc.check_constructed(case["tree"], case["dmin"], case["dmax"], case["vector_cost"])
    # every CU of the expected tree refines to SATD 0 at its vector
    nodes = case["refined"]["nodes"]
    for k, (vx, vy) in ((2, tc.PAN), (3, tc.PAN), (6, tc.PAN), (9, tc.PAN), (10, tc.PAN)) + tuple((21 + (i >> 1) * 8 + (i & 1), v) for i, v in enumerate(tc.MOVES_8)):
        assert (nodes["satd_best"][0, k], nodes["mvx"][0, k], nodes["mvy"][0, k]) == (0, 4 * vx, 4 * vy), k
    # the library's host function on the same records
    dmin, dmax, tree = capi.p_tree_select(case["shapes"], tc.W, tc.H, with_tree=True)
    tr.same(tree, case["tree"])
    assert np.array_equal(dmin, case["dmin"]) and np.array_equal(dmax, case["dmax"])


def test_constructed_motions_through_the_centred_chain(oracle):
    """one coarse centre per CTU moves the predictor, so costs change -- the map does not, and the root's tree is still the sum of its 15 vector costs"""
    import p_tree_cases as tc
    case = tc.centred_case(oracle)
    assert (int(case["centres"]["mvx"][0]), int(case["centres"]["mvy"][0])) != (0, 0)
    tc.check_constructed(case["tree"], case["dmin"], case["dmax"], case["vector_cost"])
    assert np.array_equal(case["dmin"], tc.constructed_case(oracle)["dmin"])
    assert case["tree"]["cost_tree"][0, 0] != tc.constructed_case(oracle)["tree"]["cost_tree"][0, 0]


def test_the_selection_s_constructed_pair_through_the_tree(oracle):
    """pu_shape_cases: its three constructed CUs are cheaper as two PUs than as one, and cheaper than their four children: none of them splits"""
    import pu_shape_cases as pc
    case = pc.constructed_case(oracle)
    rec, dmin, dmax = tr.select(case["rec"][None], pc.W, pc.H)
    assert np.array_equal(dmin, dmax)
    for c, k in (pc.CU_2NxN, pc.CU_nLx2N, pc.CU_Nx2N_16):
        assert rec["cost_own"][0, c, k] == case["rec"]["cost_best"][c, k]
    for c, k in (pc.CU_2NxN, pc.CU_nLx2N):
        assert rec["flags"][0, c, k] & T and not rec["flags"][0, c, k] & S, (k, rec[0, c, k])
    m = dmin[0, 0].reshape(16, 16)
    assert (m[8:16, 8:16] == 1).all() and (m[0:8, 0:8] == 1).all()
    hmin, hmax = capi.p_tree_select(case["rec"], pc.W, pc.H)
    assert np.array_equal(hmin, dmin[0]) and np.array_equal(hmax, dmax[0])
