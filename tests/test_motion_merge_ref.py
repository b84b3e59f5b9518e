"""Pins tests/motion_merge_ref.py, the Python restatement the merge kernel and the tree decision with merge costs are held to (no GPU needed): the
candidate list on hand-made records (every availability reason, HM's pruning pairs, lengths, bits, ties), the distortion against what the reference's own
xPatternSearchFracDIF recorded, a picture made by the filter itself, a pair with two motions through every CPU restatement of the chain, and the one
rule that extends the tree."""
import numpy as np

import motion_golden as gold
import motion_merge_cases as mc
import motion_merge_ref as mg
import motion_refine_ref as mr
import p_tree_ref as tr

V = ((4, -8), (12, 0), (-3, 5), (7, 7), (-20, 1))       # five different vectors within the reach of max_range 8
OK = 100                                                # a cost that is no marker


def cands(**kw):
    """L=, A=, AR=, BL=, AL= vectors -> build_list's input with available records"""
    return [None if kw.get(n) is None else (OK,) + tuple(kw[n]) for n in ("L", "A", "AR", "BL", "AL")]


# ---- the candidate list --------------------------------------------------------------------------------------------------------------------------

def test_positions_on_the_grid_inside_the_band():
    W, H = 200, 136                 # 4 x 3 CTUs, ragged by 8 both ways: 3 x 2 whole 64x64 nodes, 6 x 4 whole 32x32 nodes, 25 x 17 whole 8x8 nodes
    whole = (0, 3)
    # the grid's edges: no L / BL / AL in the first column, no A / AR / AL in the first row
    assert mg.neighbours(W, H, whole, 0, 0, 0) == [None] * 5
    assert mg.neighbours(W, H, whole, 0, 0, 1) == [None, (0, 0), (1, 0), None, None]
    assert mg.neighbours(W, H, whole, 0, 1, 0) == [(0, 0), None, None, None, None]        # BL = (0, 1): a later CTU
    assert mg.neighbours(W, H, whole, 0, 1, 1) == [(4, 0), (1, 0), (2, 0), None, (0, 0)]
    # not INSIDE: the 64x64 node of CTU column 3 crosses the edge, so (2, 1) has no AR; row 2 crosses it, so nothing of it is ever a BL
    assert mg.neighbours(W, H, whole, 0, 2, 1) == [(5, 0), (2, 0), None, None, (1, 0)]
    # ... at level 3 the ragged CTU's first column is inside: 8x8 node (24, 1) is node (0, 1) of CTU 3; its AR (25, 0) is not
    assert mg.inside(W, H, 3, 24, 16) and not mg.inside(W, H, 3, 25, 0) and not mg.inside(W, H, 3, 0, 17)
    n = mg.neighbours(W, H, whole, 3, 24, 1)
    assert n[mg.L] == (2, mg.node_index(3, 7, 1)) and n[mg.A] == (3, mg.node_index(3, 0, 0)) and n[mg.AR] is None
    # the band is a slice: in its first CTU row nothing comes from above, and the last row's BL never leaves it
    assert mg.neighbours(W, H, (1, 3), 0, 1, 1) == [(4, 0), None, None, None, None]
    assert mg.neighbours(W, H, (1, 2), 1, 2, 2) == [(4, mg.node_index(1, 1, 0)), None, None, (4, mg.node_index(1, 1, 1)), None]
    assert mg.neighbours(W, H, (0, 3), 1, 2, 2)[mg.A] == (1, mg.node_index(1, 0, 1))
    # inside a CTU row of the band the second node row has its A again
    assert mg.neighbours(W, H, (1, 2), 1, 2, 3)[mg.A] == (5, mg.node_index(1, 0, 0))


# AR and BL of the four 32x32 nodes of a CTU with CTUs all around, written out by hand (z-order 0 1 / 2 3):
#   (0, 0): AR lies in the CTU above, BL in the CTU to the left: both coded;      (1, 0): AR in the CTU above right: coded; BL = (0, 1), z 2: not yet
#   (0, 1): AR = (1, 0), z 1: coded; BL in the CTU below left: not yet;            (1, 1): AR in the CTU to the right, BL in the CTU below: not yet
LEVEL1 = {(0, 0): (True, True), (1, 0): (True, False), (0, 1): (True, False), (1, 1): (False, False)}


def test_coding_order_decides_ar_and_bl(oracle):
    W = H = 192                      # 3 x 3 whole CTUs; the nodes of the middle one have neighbours on every side
    r2z, z2r = np.zeros(256, np.uint16), np.zeros(256, np.uint16)
    oracle.fho_init_scan_tables(r2z, z2r)
    for lvl in (1, 2, 3):
        n, units = 1 << lvl, 16 >> lvl

        def coded_before(x, y, bx, by):
            """HM's order for the same-size CU at (x, y) of this CTU's grid -- or beyond it -- against the CU at (bx, by)"""
            if y < 0:
                return True                       # the CTU row above, above right included
            if y >= n or x >= n:
                return False                      # the CTUs to the right and below
            if x < 0:
                return True                       # the CTU to the left, same row
            return r2z[y * units * 16 + x * units] < r2z[by * units * 16 + bx * units]

        for by in range(n):
            for bx in range(n):
                got = mg.neighbours(W, H, (0, 3), lvl, n + bx, n + by)
                exp = (coded_before(bx + 1, by - 1, bx, by), coded_before(bx - 1, by + 1, bx, by))
                assert (got[mg.AR] is not None, got[mg.BL] is not None) == exp, (lvl, bx, by)
                if lvl == 1:
                    assert exp == LEVEL1[(bx, by)]
                assert got[mg.L] is not None and got[mg.A] is not None and got[mg.AL] is not None      # always coded before
                # the z-index is the oracle's scan order
                assert mg.z_index(bx, by) == r2z[by * units * 16 + bx * units] // (units * units)
    # where the position is addressable, it names the node that holds it
    got = mg.neighbours(W, H, (0, 3), 2, 4, 4)
    assert got == [(3, mg.node_index(2, 3, 0)), (1, mg.node_index(2, 0, 3)), (1, mg.node_index(2, 1, 3)), (3, mg.node_index(2, 3, 1)), (0, mg.node_index(2, 3, 3))]


def test_markers_and_the_reach():
    a, b = V[0], V[1]
    assert mg.build_list(cands(L=a, A=b), 8) == [(mg.L, a), (mg.A, b), (mg.ZERO, (0, 0))]
    # a marked record is no candidate, whatever its vector says -- and prunes nothing
    c = cands(L=a, A=a)
    c[mg.L] = (mg.MARK,) + a
    assert mg.build_list(c, 8) == [(mg.A, a), (mg.ZERO, (0, 0))]
    # the reach of max_range R is 4 R + 3 quarter samples in either component and either direction; one beyond is no candidate
    for R in (1, 8, 33, 64):
        far = 4 * R + 3
        for v in ((far, 0), (0, far), (-far, -far)):
            assert mg.build_list(cands(L=v), R) == [(mg.L, v), (mg.ZERO, (0, 0))]
        for v in ((far + 1, 0), (0, -far - 1), (far, far + 1)):
            assert mg.build_list(cands(L=v, A=a if R >= 8 else (1, 1)), R)[0][0] == mg.A
            assert mg.build_list(cands(L=v), R) == [(mg.ZERO, (0, 0))]
    # a zero vector from a neighbour is a candidate like any other, and the closing zero is not pruned against it
    assert mg.build_list(cands(L=(0, 0)), 8) == [(mg.L, (0, 0)), (mg.ZERO, (0, 0))]


def test_pruning_pairs_al_and_lengths():
    a, b, c, d, e = V
    src = lambda lst: [s for s, _ in lst]
    # the four pairs, each firing and not firing
    assert src(mg.build_list(cands(L=a, A=a), 8)) == [mg.L, mg.ZERO] and src(mg.build_list(cands(L=a, A=b), 8)) == [mg.L, mg.A, mg.ZERO]
    assert src(mg.build_list(cands(A=a, AR=a), 8)) == [mg.A, mg.ZERO] and src(mg.build_list(cands(A=a, AR=b), 8)) == [mg.A, mg.AR, mg.ZERO]
    assert src(mg.build_list(cands(L=a, BL=a), 8)) == [mg.L, mg.ZERO] and src(mg.build_list(cands(L=a, BL=b), 8)) == [mg.L, mg.BL, mg.ZERO]
    assert src(mg.build_list(cands(L=a, AL=a), 8)) == [mg.L, mg.ZERO] and src(mg.build_list(cands(A=a, AL=a), 8)) == [mg.A, mg.ZERO]
    assert src(mg.build_list(cands(L=a, A=b, AL=c), 8)) == [mg.L, mg.A, mg.AL, mg.ZERO]
    # only HM's pairs: AR is not compared with L, BL not with A or AR, AL not with AR or BL
    assert src(mg.build_list(cands(L=a, AR=a), 8)) == [mg.L, mg.AR, mg.ZERO]
    assert src(mg.build_list(cands(A=a, BL=a), 8)) == [mg.A, mg.BL, mg.ZERO]
    assert src(mg.build_list(cands(AR=a, BL=a, AL=a), 8)) == [mg.AR, mg.BL, mg.AL, mg.ZERO]
    # a pair fires against an AVAILABLE neighbour, admitted or not: A equals L and is pruned; AR equals A and is pruned against it all the same
    assert src(mg.build_list(cands(L=a, A=a, AR=a), 8)) == [mg.L, mg.ZERO]
    # AL is admitted at length 3 and refused at length 4
    assert src(mg.build_list(cands(L=a, A=b, AR=c, AL=e), 8)) == [mg.L, mg.A, mg.AR, mg.AL, mg.ZERO]
    assert src(mg.build_list(cands(L=a, A=b, AR=c, BL=d, AL=e), 8)) == [mg.L, mg.A, mg.AR, mg.BL, mg.ZERO]
    # lengths 1..5; a full list has no zero vector
    assert [len(mg.build_list(cands(**dict(list(zip(("L", "A", "AR", "AL"), V))[:n])), 8)) for n in range(5)] == [1, 2, 3, 4, 5]
    assert src(mg.build_list(cands(L=a, A=b, AR=c, AL=e), 8))[-1] == mg.ZERO and len(mg.build_list(cands(L=a, A=b, AR=c, BL=d), 8)) == 5


def test_bits_and_ties():
    assert [mg.index_bits(i) for i in range(5)] == [1, 2, 3, 4, 4]
    sl = 10.0
    assert [mg.bit_cost(b, sl) for b in range(5)] == [0, 10, 20, 30, 40]
    entries = mg.build_list(cands(L=V[0], A=V[1], AR=V[2], BL=V[3]), 8)
    assert len(entries) == 5 and entries[4][0] == mg.ZERO
    # equal costs: the earlier entry wins (20 + 10 = 10 + 20 = 0 + 30)
    assert mg.choose(entries, [20, 10, 0, 50, 50], sl) == (20, 30, V[0][0], V[0][1], 0, 5, mg.L, 0)
    assert mg.choose(entries, [21, 10, 0, 50, 50], sl) == (10, 30, V[1][0], V[1][1], 1, 5, mg.A, 0)
    # entry 4 costs four bits, not five: it ties with entry 3 at equal distortion, and the earlier one wins; one less and it wins
    assert mg.choose(entries, [99, 99, 99, 7, 7], sl)[4] == 3
    assert mg.choose(entries, [99, 99, 99, 7, 6], sl) == (6, 46, 0, 0, 4, 5, mg.ZERO, 0)
    assert mg.choose(entries[:1] + [(mg.ZERO, (0, 0))], [5, 0], sl) == (5, 15, V[0][0], V[0][1], 0, 2, mg.L, 0)
    assert mg.choose(entries[:1] + [(mg.ZERO, (0, 0))], [11, 0], sl) == (0, 20, 0, 0, 1, 2, mg.ZERO, 0)


# ---- the distortion, pinned to the reference ----------------------------------------------------------------------------------------------------------

def test_satd_at_the_references_own_vectors(oracle):
    """for every valid square node of every case of the quarter-sample golden: the distortion at the vector the reference's xPatternSearchFracDIF returned
    is the one the file holds for it"""
    checked = 0
    for case in gold.frac_cases():
        planes = mr.Planes(case.ref.astype(np.int64), case.bd, case.R + 8)
        flat = np.ascontiguousarray(case.cur).reshape(-1)
        rec = case.records("nodes")
        cw = (case.W + 63) // 64
        for i, c in enumerate(case.ctus):
            for k in range(85):
                lvl, bx, by = mr.node_geometry(k)
                n = 64 >> lvl
                x0, y0 = (c % cw) * 64 + bx * n, (c // cw) * 64 + by * n
                r = rec[i, k]
                assert (r["cost_best"] == gold.MARKER) == (x0 + n > case.W or y0 + n > case.H)
                if r["cost_best"] != gold.MARKER:
                    assert mg.satd_at(oracle, planes, flat, 0, case.W, x0, y0, n, (int(r["mvx"]), int(r["mvy"]))) == int(r["satd_best"]), (case, c, k)
                    checked += 1
    assert checked == gold.FRAC_COUNTS["nodes"]


# ---- constructed pictures -------------------------------------------------------------------------------------------------------------------------------

def test_a_half_sample_picture_merges_at_no_distortion(oracle):
    for bd, fx, fy, mv in mc.HALF_CASES:
        case = mc.half_sample_case(bd, fx, fy, mv)
        flat = np.ascontiguousarray(case["cur"].astype(np.int16)).reshape(-1)
        got = mg.expected(oracle, flat, 0, mc.HALF_W, case["ref"], mc.HALF_W, mc.HALF_H, bd, mc.HALF_QP, case["refined"], 8, planes=case["planes"])
        mc.check_half_sample(got, case["q"], mg.bit_cost(1, mr.sqrt_lambda(oracle, mc.HALF_QP, bd)))


def test_two_motions_split_at_a_ctu_boundary(oracle):
    case = mc.two_motion_case(oracle)
    rec, dmin, dmax = case["merged"]
    mc.check_two_motions(case["refined"]["nodes"], case["merge"], rec, dmin, dmax, case["vector_cost"], case["c"])
    # without the merge stage the same nodes pay for their vectors, and bit 6 never appears
    plain = case["plain"][0]
    assert [int(v) for v in plain["cost_own"][:, 0]] == [case["vector_cost"](c, *v) for c, v in enumerate((mc.V1, mc.V2, mc.V2))]
    assert not (plain["flags"] & mg.MERGED).any() and (rec["cost_own"] <= plain["cost_own"]).all()
    assert int(rec["cost_own"][2, 0]) < int(plain["cost_own"][2, 0])


def test_two_motions_through_the_centred_chain(oracle):
    """the same pair around one coarse centre per CTU, the merge stage at max_range 64 on absolute vectors: the same story, with every explicit vector priced
    against its CTU's centre and the inherited ones priced as before"""
    case = mc.two_motion_centred_case(oracle)
    P = [(int(case["centres"]["mvx"][c]), int(case["centres"]["mvy"][c])) for c in range(3)]
    assert all(abs(p[0]) <= 4 and abs(p[1]) <= 4 and p[0] % 4 == 0 and p[1] % 4 == 0 for p in P), P
    rec, dmin, dmax = case["merged"]
    mc.check_two_motions(case["refined"]["nodes"], case["merge"], rec, dmin, dmax, case["vector_cost"], case["c"])
    plain = case["plain"][0]
    assert [int(v) for v in plain["cost_own"][:, 0]] == [case["vector_cost"](c, *v) for c, v in enumerate((mc.V1, mc.V2, mc.V2))]
    assert not (plain["flags"] & mg.MERGED).any() and (rec["cost_own"] <= plain["cost_own"]).all()
    # the merge records do not depend on the centres at all where the refined vectors are the same: the 64x64 nodes' equal the zero-centred chain's
    wide = mc.two_motion_case(oracle)
    for f in mg.MDT.names:
        assert np.array_equal(case["merge"][f][:, 0], wide["merge"][f][:, 0]), f


# ---- the tree's one new rule --------------------------------------------------------------------------------------------------------------------------------

def test_tree_own_cost_is_the_smaller_available_one():
    W = H = 64
    shapes = np.full((1, 1, 85), 1000, np.uint32)
    merge = np.full((1, 1, 85), mg.MARK, np.uint32)
    base = tr.select(shapes, W, H)
    # all merge costs MARK: nothing changes, bit 6 nowhere
    got = mg.tree_select(shapes, merge, W, H)
    assert all(g.tobytes() == b.tobytes() for g, b in zip(got, base))
    # the four combinations on the root and on a leaf
    for k in (0, 84):
        for s, m, own, bit in ((1000, 999, 999, True), (1000, 1000, 1000, False), (1000, 1001, 1000, False), (mg.MARK, 5, 5, True), (7, mg.MARK, 7, False),
                               (mg.MARK, mg.MARK, mg.MARK, False)):
            sh, me = shapes.copy(), merge.copy()
            sh[0, 0, k], me[0, 0, k] = s, m
            rec = mg.tree_select(sh, me, W, H)[0][0, 0]
            assert rec["cost_own"][k] == own and bool(rec["flags"][k] & mg.MERGED) == bit and bool(rec["flags"][k] & tr.OWN_AVAILABLE) == (own != mg.MARK), (k, s, m)
    # a cheaper merged root stops the split that the plain tree makes: children 4 x 1000 against own 4001, then against a merge cost of 3999
    sh = shapes.copy()
    sh[0, 0, 0] = 4001
    sh[0, 0, 1:5] = 1000
    sh[0, 0, 5:] = 100000
    me = merge.copy()
    assert tr.select(sh, W, H)[1][0, 0].max() == 1
    me[0, 0, 0] = 3999
    rec, dmin, dmax = mg.tree_select(sh, me, W, H)
    assert dmax[0, 0].max() == 0 and rec["cost_tree"][0, 0, 0] == 3999 and rec["flags"][0, 0, 0] & tr.STOP_SURE
    # bit 6 is a statement about INSIDE nodes: a crossing or absent node never carries it
    Wr, Hr = 40, 24
    me = np.zeros((1, 1, 85), np.uint32)
    rec = mg.tree_select(np.full((1, 1, 85), 1000, np.uint32), me, Wr, Hr)[0][0, 0]
    for k in range(85):
        assert bool(rec["flags"][k] & mg.MERGED) == tr.geometry(k, Wr, Hr)[0], k
