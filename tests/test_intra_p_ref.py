"""tests/intra_p_ref.py, the Python restatement of the intra stage of P pictures and of the tree that takes its costs, held to hand-computed cases
(no GPU needed).  The library is not asked here, except for one thing the restatement cannot know by itself: that capi.INTRA_P_DTYPE has the pinned layout.

The draw (intra_p_ref.draw: random records on 200 x 136 and 100 x 76, seeds 823 + W) has DRAW_PICTURES = 14 pictures per size: the smallest number for which
the restatement alone shows every case of both definitions at every level it can occur at, at least 8 times over the two sizes together.  The rarest case is
a calm root whose intra cost is smaller and is withheld (8 times at 14 pictures; 6 at 13, 4 at 12); the next rarest are an unpriced root (10) and an intra
cost one below the root's inter cost (11)."""
import math

import numpy as np
import pytest

import intra_p_ref as ip
import motion_merge_ref as mg
import motion_skip_ref as sk
import p_tree_ref as pt
from fasthevc_amd import capi

MARK, SAT = ip.MARK, ip.SAT
C32 = {2: 15, 3: 22, 6: 45}          # sqrt(lambda(32)) = sqrt(0.57 * 2^(20 / 3)) = 7.6097..: floor of 15.2, 22.8, 45.7


def test_the_record_layout():
    assert ip.IDT.itemsize == 16 and [ip.IDT.fields[n][1] for n in ip.IDT.names] == [0, 4, 8, 12, 13]
    assert ip.IDT.names == ("satd_best", "cost_best", "modes", "part", "pad")


def test_bits_over_all_256_mode_bytes():
    assert [ip.bits(m) for m in range(256)] == [2, 3] + [6] * 24 + [3] + [6] * 229
    # only the low byte of the mode dword counts
    assert ip.price(100, 0x12345600, C32) == 115 and ip.price(100, 0xFFFFFF1A, C32) == 122 and ip.price(100, 0x00000100 | 7, C32) == 145


@pytest.mark.parametrize("qp, sl", [(0, 0.18874586), (22, 2.39692302), (32, 7.60975626), (51, 68.33330081)])
def test_bit_costs_against_the_formula_of_mv_bits_cost(qp, sl):
    """sl: sqrt(0.57 * 2^((qp - 12) / 3)) to 8 places (qp 0 and 51 from exact powers of two: sqrt(0.57 / 16), sqrt(0.57 * 8192)); c[b] = (uint32_t)((65536 sl * b) / 65536.0)"""
    assert abs(ip.sqrt_lambda(qp) - sl) < 1e-7
    ml = 65536.0 * math.sqrt(0.57 * math.pow(2.0, (qp - 12.0) / 3.0))
    c = ip.bit_costs(qp)
    assert c == {b: int((ml * b) / 65536.0) for b in (2, 3, 6)} == {b: int(math.floor(sl * b)) for b in (2, 3, 6)}
    assert {0: {2: 0, 3: 0, 6: 1}, 22: {2: 4, 3: 7, 6: 14}, 32: C32, 51: {2: 136, 3: 204, 6: 409}}[qp] == c


def fields(r):
    """a record of the restatement's output as the tuple node_record gives"""
    return int(r["satd_best"]), int(r["cost_best"]), tuple(r["modes"].tolist()), int(r["part"]), tuple(r["pad"].tolist())


A72, NONE = (50, 72, (1, 1, 1, 1), 0, (0, 0, 0)), ip.MARKER


def one_ctu(node_satd=1000, node_mode=0, pus=((100, 0),) * 4, k=21):
    """a whole CTU of marker first-pass records, but node k and its four PUs -> (first, first4) as lists of (satd, mode)"""
    first, first4 = [(MARK, 255)] * 85, [(MARK, 255)] * 256
    first[k] = (node_satd, node_mode)
    _, x, y = pt.node_pos(k)
    for j, pu in enumerate(pus):
        first4[(2 * y + (j >> 1)) * 16 + 2 * x + (j & 1)] = pu
    return first, first4


def test_nxn_against_2Nx2N_by_hand():
    # four PUs of satd 100, modes 0, 1, 26, 9: prices 115, 122, 122, 145 = 504; satd 400
    pus = ((100, 0), (100, 1), (100, 26), (100, 9))
    k = pt.node_id(3, 5, 2)
    for satd, exp in ((490, (400, 504, (0, 1, 26, 9), 1, (0, 0, 0))),          # 2Nx2N 505: NxN one less
                      (489, (489, 504, (0, 0, 0, 0), 0, (0, 0, 0))),           # a tie: 2Nx2N stays
                      (488, (488, 503, (0, 0, 0, 0), 0, (0, 0, 0)))):          # NxN one more
        first, first4 = one_ctu(satd, 0, pus, k)
        assert ip.node_record(k, 64, 64, first, first4, C32) == exp
        assert ip.node_record(k, 64, 64, first, None, C32) == (satd, satd + 15, (0, 0, 0, 0), 0, (0, 0, 0))
    # one unpriced PU of the four: no NxN candidate, however cheap the other three
    first, first4 = one_ctu(5000, 30, ((0, 0), (0, 0), (MARK, 0), (0, 0)), k)
    assert ip.node_record(k, 64, 64, first, first4, C32) == (5000, 5045, (30, 30, 30, 30), 0, (0, 0, 0))
    # 2Nx2N unavailable with NxN available, and neither
    first, first4 = one_ctu(MARK, 3, pus, k)
    assert ip.node_record(k, 64, 64, first, first4, C32) == (400, 504, (0, 1, 26, 9), 1, (0, 0, 0))
    assert ip.node_record(k, 64, 64, first, None, C32) == ip.MARKER
    first, first4 = one_ctu(MARK, 3, ((1, 1), (MARK, 1), (1, 1), (1, 1)), k)
    assert ip.node_record(k, 64, 64, first, first4, C32) == ip.MARKER
    # the PUs of the 8x8 node at (x, y) are (2x, 2y), (2x + 1, 2y), (2x, 2y + 1), (2x + 1, 2y + 1): the neighbours' PUs are not looked at
    first, first4 = one_ctu(MARK, 3, pus, k)
    first4[(2 * 2) * 16 + 2 * 5 + 2] = (0, 0)
    assert ip.node_record(k, 64, 64, first, first4, C32)[1] == 504
    # upper levels never look at the 4x4 records
    first, first4 = one_ctu(700, 26, pus, 3)
    assert ip.node_record(3, 64, 64, first, first4, C32) == (700, 722, (26, 26, 26, 26), 0, (0, 0, 0))


def test_saturation_of_the_price_and_of_the_four_sum():
    k = 21
    for satd, exp in ((SAT - 16, SAT - 1), (SAT - 15, SAT), (SAT - 14, SAT), (SAT, SAT)):
        first, _ = one_ctu(satd, 0, k=k)
        assert ip.node_record(k, 64, 64, first, None, C32) == (satd, exp, (0, 0, 0, 0), 0, (0, 0, 0))
    # four PUs whose prices add up to just below 2^32 - 2, to it, and beyond: q = (2^32 - 2 - 60) / 4 = 1073741808.5
    q = (SAT - 60) // 4                                        # 1073741808: four prices of q + 15 = SAT - 2
    for extra, cost in ((0, SAT - 2), (1, SAT - 1), (2, SAT), (3, SAT), (1 << 20, SAT)):
        first, first4 = one_ctu(MARK, 0, ((q, 0), (q, 0), (q, 0), (q + extra, 0)), k)
        assert ip.node_record(k, 64, 64, first, first4, C32) == (min(4 * q + extra, SAT), cost, (0, 0, 0, 0), 1, (0, 0, 0))
    # the satd saturates on its own: satds near 2^32 whose prices are each SAT already
    first, first4 = one_ctu(MARK, 0, ((SAT, 0),) * 4, k)
    assert ip.node_record(k, 64, 64, first, first4, C32) == (SAT, SAT, (0, 0, 0, 0), 1, (0, 0, 0))
    # a saturated NxN cost never beats a saturated 2Nx2N price (strict), and loses to any smaller one
    first, first4 = one_ctu(SAT, 0, ((SAT, 0),) * 4, k)
    assert ip.node_record(k, 64, 64, first, first4, C32)[3] == 0


@pytest.mark.parametrize("size", [8, 12, 36, 40, 64])
def test_every_geometry_class(size):
    """a size x size picture of priced records everywhere: exactly the INSIDE nodes carry a record"""
    first = np.zeros((1, 1, 85), ip.NDT)
    first["satd"], first["mode"] = 50, 1
    out = ip.stage(first, None, size, size, 32)[0, 0]
    count = 0
    for k in range(85):
        l, x, y = pt.node_pos(k)
        s = 64 >> l
        inside = (x + 1) * s <= size and (y + 1) * s <= size
        assert pt.geometry(k, size, size)[0] == inside
        count += inside
        assert fields(out[k]) == (A72 if inside else NONE), k
    # whole CUs of 64 / 32 / 16 / 8 samples in a size x size picture
    assert count == sum((size // (64 >> l)) ** 2 for l in range(4)) == {8: 1, 12: 1, 36: 1 + 4 + 16, 40: 1 + 4 + 25, 64: 85}[size]


def test_every_geometry_class_nxn_wins_inside_only():
    first, first4 = np.zeros((1, 1, 85), ip.NDT), np.zeros((1, 1, 256), ip.NDT)
    first["satd"], first["mode"], first4["satd"], first4["mode"] = 50, 1, 1, 0      # 2Nx2N 72; NxN 4 * 16 = 64
    first4["satd"][0, 0, 0] = 3                                                         # but the first 8x8 node: 66
    first4["satd"][0, 0, 17] = 7                                                        # ... 72: a tie, 2Nx2N stays
    for size in (8, 12, 36, 40, 64):
        out = ip.stage(first, first4, size, size, 32)[0, 0]
        for k in range(21, 85):
            inside = pt.geometry(k, size, size)[0]
            exp = NONE if not inside else (A72 if k == 21 else (4, 64, (0, 0, 0, 0), 1, (0, 0, 0)))
            assert fields(out[k]) == exp, (size, k)
    first4["satd"][0, 0, 17] = 6
    assert fields(ip.stage(first, first4, 64, 64, 32)[0, 0, 21]) == (11, 71, (0, 0, 0, 0), 1, (0, 0, 0))


# ---- the tree -----------------------------------------------------------------------------------------------------------------------------------------

def tree_inputs(k, inter_shape, inter_merge, intra_cost, flags=0):
    """a whole CTU in which every node costs 10 to code, merge and intra unavailable -- but node k"""
    shapes, merge, intra, skip = [10] * 85, [MARK] * 85, [MARK] * 85, [0] * 85
    shapes[k], merge[k], intra[k], skip[k] = inter_shape, inter_merge, intra_cost, flags
    return shapes, merge, skip, intra


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_intra_one_less_equal_and_one_more_than_inter(level):
    k = pt.node_id(level, (1 << level) - 1, 0)
    for shape, merge in ((5000, MARK), (6000, 5000), (5000, 5000), (MARK, 5000)):
        for intra_cost, taken in ((4999, True), (5000, False), (5001, False), (MARK, False)):
            s, m, f, i = tree_inputs(k, shape, merge, intra_cost)
            rec, dmin, dmax = ip.tree_ctu(s, m, f, 3, i, 64, 64)
            ref = sk.tree_ctu(s, m, f, 3, 64, 64)
            assert int(rec["cost_own"][k]) == (4999 if taken else 5000) and int(rec["pad"][k, 0]) == int(taken) and int(rec["pad"][k, 1]) == 0
            assert bool(rec["flags"][k] & mg.MERGED) == (merge < shape), "bit 6 keeps its meaning"
            if not taken:
                assert rec.tobytes() == ref[0].tobytes() and np.array_equal(dmin, ref[1]) and np.array_equal(dmax, ref[2])
            else:
                assert (rec["pad"][:, 0] != 0).sum() == 1
    # both inter costs unavailable: any intra cost is taken, and the node becomes available
    s, m, f, i = tree_inputs(k, MARK, MARK, 77)
    rec, _, _ = ip.tree_ctu(s, m, f, 0, i, 64, 64)
    assert int(rec["cost_own"][k]) == 77 and rec["flags"][k] & pt.OWN_AVAILABLE and rec["pad"][k, 0] == 1


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_a_calm_node_withholds_a_smaller_intra_cost(level):
    """own: merge 5000 < selection 6000, a masked zero bit; intra 100.  The children (10 each, 40 together) would be cheaper than 5000 on levels 0..2."""
    k = pt.node_id(level, 0, (1 << level) - 1)
    for flags, mask, calm in ((sk.ZERO_HALF, 3, True), (sk.ZERO_HALF, 2, True), (sk.ZERO_HALF, 1, False), (sk.ZERO_HALF, 0, False), (sk.ZERO_PLAIN, 1, True),
                              (0, 3, False), (0xFC, 3, False)):
        s, m, f, i = tree_inputs(k, 6000, 5000, 100, flags)
        rec, dmin, dmax = ip.tree_ctu(s, m, f, mask, i, 64, 64)
        assert int(rec["cost_own"][k]) == (5000 if calm else 100) and int(rec["pad"][k, 0]) == (0 if calm else 1) and rec["flags"][k] & mg.MERGED
        if level < 3:
            # withheld and not descended (EarlyCU, as today); taken: an ordinary node whose own cost is 100
            assert bool(rec["flags"][k] & sk.SKIPPED) == calm and (not calm or (rec["flags"][k] & pt.STOP_SURE and int(rec["cost_tree"][k]) == 5000))
            kids = int(rec["cost_kids"][k])
            assert kids == 40                     # every child's tree is its own 10: its own children would cost 40
            assert calm or int(rec["cost_tree"][k]) == min(100, kids)
        else:
            assert not rec["flags"][k] & sk.SKIPPED and int(rec["cost_tree"][k]) == (5000 if calm else 100)
        if calm:
            ref = sk.tree_ctu(s, m, f, mask, 64, 64)
            assert rec.tobytes() == ref[0].tobytes() and np.array_equal(dmin, ref[1]) and np.array_equal(dmax, ref[2])
    # a node whose SELECTION cost is the smaller one is never calm, whatever its skip flags
    s, m, f, i = tree_inputs(k, 5000, 6000, 100, 3)
    assert int(ip.tree_ctu(s, m, f, 3, i, 64, 64)[0]["pad"][k, 0]) == 1


def test_an_intra_root_stops_the_tree_by_the_ordinary_rule():
    """a root whose intra cost is below the sum of its children: depth 0 everywhere, by the margins' own comparison and not by a skip"""
    s, m, f, i = tree_inputs(0, 100000, MARK, 39)
    rec, dmin, dmax = ip.tree_ctu(s, m, f, 3, i, 64, 64)
    assert int(rec["cost_kids"][0]) == 40 and int(rec["cost_tree"][0]) == 39 and rec["flags"][0] & pt.STOP_SURE and not rec["flags"][0] & sk.SKIPPED
    assert not dmin.any() and not dmax.any()
    i[0] = 41
    rec, dmin, dmax = ip.tree_ctu(s, m, f, 3, i, 64, 64)
    assert int(rec["cost_tree"][0]) == 40 and rec["flags"][0] & pt.SPLIT_SURE and rec["pad"][0, 0] == 1 and dmin.min() >= 1


def test_not_inside_nodes_never_take_intra():
    s, m, f, i = [10] * 85, [MARK] * 85, [0] * 85, [1] * 85
    rec, _, _ = ip.tree_ctu(s, m, f, 3, i, 40, 24)
    for k in range(85):
        inside = pt.geometry(k, 40, 24)[0]
        assert int(rec["pad"][k, 0]) == int(inside) and (inside or int(rec["cost_own"][k]) == MARK)


@pytest.mark.parametrize("size", ip.DRAW_SIZES)
def test_all_mark_intra_records_equal_the_skip_tree_on_the_draw(size):
    d = ip.draw(size)
    blank = ip.all_mark(d["intra"])
    for rname, mask in (("default", 0), ("r1", 3), ("r2", 1), ("r3", 2)):
        a = ip.tree_select(d["shapes"], d["merge"], d["skip"], mask, blank, *size, rule=d["rules"][rname])
        b = sk.tree_select(d["shapes"], d["merge"], d["skip"], mask, *size, rule=d["rules"][rname])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (rname, mask)
    # ... and the real intra records change something
    assert (ip.draw_tree(size, "r1", 3)[0]["pad"][..., 0] != 0).any()


def test_the_draw_shows_every_case():
    """every case of both definitions at every level it can occur at, at least 8 times over the two sizes (see the module's docstring for the number of pictures)"""
    seen = {}
    for size in ip.DRAW_SIZES:
        d = ip.draw(size)
        ip.stage_coverage(d["first"], d["first4"], d["out"], *size, ip.DRAW_QP, seen=seen)
        ip.tree_coverage(d["shapes"], d["merge"], d["skip"], d["intra"], 3, ip.draw_tree(size, "default", 3)[0], *size, seen=seen)
    taken = {}
    for size in ip.DRAW_SIZES:     # the same calm nodes with skip_mask 0: taken
        d = ip.draw(size)
        rec3, rec0 = ip.draw_tree(size, "default", 3)[0], ip.draw_tree(size, "default", 0)[0]
        ip.tree_coverage(d["shapes"], d["merge"], d["skip"], d["intra"], 0, rec0, *size, seen=taken)
        withheld = ((d["merge"]["cost_best"] < d["shapes"]["cost_best"]) & ((d["skip"]["flags"] & 3) != 0) & (d["intra"]["cost_best"] < d["merge"]["cost_best"]) &
                    ((rec3["flags"] & (pt.ABSENT | pt.CROSSING)) == 0) & ((rec3["flags"] & mg.MERGED) != 0))
        assert not (rec3["pad"][..., 0][withheld] != 0).any() and (rec0["pad"][..., 0][withheld] == 1).all()
    need = [(c, l) for c in ip.STAGE_CASES for l in range(4)] + [(c, 3) for c in ip.NXN_CASES] + [(c, l) for c in ip.TREE_CASES for l in range(4)]
    short = {k: seen.get(k, 0) for k in need if seen.get(k, 0) < 8}
    assert not short, short
    assert not any(k[0] == "calm_withheld" for k in taken)
    assert min(seen[k] for k in need) == seen[("calm_withheld", 0)] == 8, "the rarest case and its count, as the docstring states them"


# ---- the constructed pair: what is known in advance, confirmed without a GPU ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10])
def test_the_constructed_pair_intra_side(bd):
    """CTU 0 of the current picture is flat at 1 << (bd - 1), in the picture's corner: every predictor of every block is that value, every SATD 0, and the
    cheapest mode is the one of fewest bits, planar.  So every node's intra record is satd 0, mode 0, cost c[2], part 0 (NxN would cost 4 c[2]); against ANY inter
    costs above c[2] the root takes it (cost_tree == c[2], the intra bit), and both maps are 0 everywhere, since 4 c[2] is not < c[2].  CTU 1 is the
    reference displaced by half a sample: its intra costs are those of noise, far above what the GPU test finds for its inter costs."""
    from oracle import oracle_py as op
    oracle = op.load_oracle()
    cur, ref = ip.constructed_pair(bd)
    assert cur.shape == (ip.PAIR_H, ip.PAIR_W) and (cur[:, :64] == 1 << (bd - 1)).all() and cur[:, 64:].std() > (1 << bd) / 8
    first, first4 = ip.oracle_first_passes(oracle, op, cur, bd, ip.PAIR_QP)
    intra = ip.stage(first[None], first4[None], ip.PAIR_W, ip.PAIR_H, ip.PAIR_QP)[0]
    c2 = ip.bit_costs(ip.PAIR_QP)[2]
    assert c2 == 15
    assert (intra["satd_best"][0] == 0).all() and (intra["cost_best"][0] == c2).all() and (intra["modes"][0] == 0).all() and (intra["part"][0] == 0).all()
    assert intra["cost_best"][1].min() > 100 * c2
    for inter in (c2 + 1, 5000, SAT, MARK):
        rec, dmin, dmax = ip.tree_ctu([inter] * 85, [MARK] * 85, [0] * 85, 3, intra["cost_best"][0], 64, 64)
        assert int(rec["cost_tree"][0]) == c2 and rec["pad"][0, 0] == 1 and not dmin.any() and not dmax.any()
        assert (rec["pad"][:, 0] == 1).all() and (rec["cost_kids"][:21] == 4 * c2).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_the_constructed_pair_through_the_chain_restatement(bd):
    """The whole zero-centred chain of fhevc_p_tree_intra_frame on the CPU (intra_p_ref.chain: the existing restatements of search, refinement, re-pricing, both
    merge stages, merge-aware selection and skip stage, the oracle's first passes, this stage and tree) on the 128 x 64 pair at qp 32, skip_mask 3.  All the
    statements hold as written, on the picture as first drawn.  CTU 0: every intra record is satd 0, mode 0, cost c[2]; every inter cost of the CTU lies above
    c[2] (a flat block against noise), so every node takes intra, the root's cost_tree == c[2] with the intra bit, and both maps are 0.  CTU 1: every node
    refines to SATD 0 at the half-sample vector, its merge or selection cost is a few vector bits, far below the intra cost of noise: no node carries the
    intra bit, and the maps are the skip tree's (0 everywhere: the root's own cost, its vector bits, lies below the sum of its children's)."""
    from oracle import oracle_py as op
    g = ip.constructed_chain(op.load_oracle(), op, bd)
    c2 = ip.bit_costs(ip.PAIR_QP)[2]
    ip.check_constructed(g, c2)
    assert min(int(g["shapes"]["cost_best"][0].min()), int(g["merge"]["cost_best"][0].min())) > c2
    assert (g["tree"]["pad"][0, :, 0] == 1).all() and (g["tree"]["cost_kids"][0, :21] == 4 * c2).all()
    inter1 = np.minimum(g["shapes"]["cost_best"][1], g["merge"]["cost_best"][1])
    assert int(inter1.max()) < int(g["intra"]["cost_best"][1].min()), "CTU 1: every inter cost lies below every intra cost"
    assert g["tree"][1].tobytes() == g["skip_tree"][1].tobytes() and g["tree"]["flags"][1, 0] & pt.STOP_SURE and not g["dmax"][1].any()
    # with skip_mask 0 nothing is calm: the statements stand, by the costs alone
    ip.check_constructed(ip.constructed_chain(op.load_oracle(), op, bd, skip_mask=0), c2)
