"""Pins tests/motion_merge_pu_ref.py, the Python restatement the per-PU merge kernel and the selection with merge costs are held to (no GPU needed): the
five candidate nodes of a PU against a table written out by hand, HM's second-PU exclusions as a consequence of the coding-order rule, AR and BL by coding
order, bands, a random draw that makes every case of the list occur, the distortion against what the reference's own xPatternSearchFracDIF recorded for
the PUs, the constructed pictures of tests/motion_merge_cases.py, and the selection's one new rule."""
import numpy as np
import pytest

import motion_golden as gold
import motion_merge_cases as mc
import motion_merge_pu_ref as mpr
import motion_merge_ref as mg
import motion_pu_ref as mp
import motion_refine_ref as mr
import pu_shape_ref as sr

HORIZ = (0, 2, 3)          # 2NxN, 2NxnU, 2NxnD: cut by a horizontal line; 1, 4, 5 (Nx2N, nLx2N, nRx2N) by a vertical one

# The five nodes L, A, AR, BL, AL of both parts of every shape of one CU per level, in a CTU with CTUs all around (the whole picture is the band), as
# positions on the CU's level's grid RELATIVE TO THE CTU (-1: the CTU to the left / above; the CTU's own grid is 0 .. 2^level - 1), None: no candidate.
# Worked out on paper from the samples (xP - 1, yP + h - 1), (xP + w - 1, yP - 1), (xP + w, yP - 1), (xP - 1, yP + h), (xP - 1, yP - 1) and the z-order.
# Where the cut lies does not matter on the CU's own level: all three horizontal (vertical) shapes share a row.
#   node 0: the 64x64 CU.  Part 1 below the cut: A is the CU itself, AR the CTU to the right, BL the CTU below left.  Part 1 right of the cut: L is the CU
#   itself, BL the CTU below
#   node 4: the 32x32 CU at (1, 1), z 3: (0, 1) z 2, (1, 0) z 1 and (0, 0) z 0 are coded; (2, .) is the CTU to the right, (., 2) the CTU below
#   node 11: the 16x16 CU at (2, 1), z 6: (1, 1) z 3, (2, 0) z 4, (3, 0) z 5, (1, 0) z 1 are coded; (1, 2) z 9, (3, 1) z 7, (2, 2) z 12 are not
#   node 42: the 8x8 CU at (5, 2), z 25: (4, 2) z 24, (5, 1) z 19, (6, 1) z 22, (4, 1) z 18 are coded; (4, 3) z 26, (6, 2) z 28, (5, 3) z 27 are not
TABLE = {
    0: {("h", 0): [(-1, 0), (0, -1), (1, -1), (-1, 0), (-1, -1)], ("h", 1): [(-1, 0), None, None, None, (-1, 0)],
        ("v", 0): [(-1, 0), (0, -1), (0, -1), None, (-1, -1)], ("v", 1): [None, (0, -1), (1, -1), None, (0, -1)]},
    4: {("h", 0): [(0, 1), (1, 0), None, (0, 1), (0, 0)], ("h", 1): [(0, 1), None, None, None, (0, 1)],
        ("v", 0): [(0, 1), (1, 0), (1, 0), None, (0, 0)], ("v", 1): [None, (1, 0), None, None, (1, 0)]},
    11: {("h", 0): [(1, 1), (2, 0), (3, 0), (1, 1), (1, 0)], ("h", 1): [(1, 1), None, None, None, (1, 1)],
         ("v", 0): [(1, 1), (2, 0), (2, 0), None, (1, 0)], ("v", 1): [None, (2, 0), (3, 0), None, (2, 0)]},
    42: {("h", 0): [(4, 2), (5, 1), (6, 1), (4, 2), (4, 1)], ("h", 1): [(4, 2), None, None, None, (4, 2)],
         ("v", 0): [(4, 2), (5, 1), (5, 1), None, (4, 1)], ("v", 1): [None, (5, 1), (6, 1), None, (5, 1)]},
}
ALL_PUS = [("pu", e, ksp) for e, ksp in enumerate(mp.covered())] + [("small", e, ksp) for e, ksp in enumerate(mpr.ps.covered())]


def quadtree_order(lvl):
    """{(x, y): position} of the 2^lvl x 2^lvl CUs of a CTU in coding order, by walking the quad-tree -- not by interleaving bits"""
    def walk(x, y, n):
        if n == 1:
            return [(x, y)]
        h = n // 2
        return walk(x, y, h) + walk(x + h, y, h) + walk(x, y + h, h) + walk(x + h, y + h, h)
    return {pos: i for i, pos in enumerate(walk(0, 0, 1 << lvl))}


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------------

def test_the_five_nodes_of_every_pu_of_an_interior_ctu():
    W = H = 192                      # 3 x 3 whole CTUs; CTU 4 has CTUs all around
    cw, c = 3, 4
    assert len(ALL_PUS) == 508
    tabled = 0
    for family, e, (k, s, p) in ALL_PUS:
        lvl, (gx, gy), (x, y, w, h) = mpr.pu_geometry(W, c, k, s, p)
        n, size = 1 << lvl, 64 >> lvl
        got = mpr.candidates(W, H, (0, 3), c, k, s, p)
        # whatever is named holds its sample, lies on the CU's level and is no later in coding order than the CU
        for (sx, sy), nb in zip(mpr.samples(x, y, w, h), got):
            if nb is not None:
                nl, nbx, nby = mr.node_geometry(nb[1])
                nx0, ny0 = (nb[0] % cw) * 64 + nbx * size, (nb[0] // cw) * 64 + nby * size
                assert nl == lvl and nx0 <= sx < nx0 + size and ny0 <= sy < ny0 + size, (k, s, p)
                assert nb[0] < c or (nb[0] == c and mg.z_index(nbx, nby) < mg.z_index(gx - n, gy - n)), (k, s, p)
        if k in TABLE:
            exp = TABLE[k][("h" if s in HORIZ else "v", p)]
            rel = [None if nb is None else ((nb[0] % cw - 1) * n + mr.node_geometry(nb[1])[1], (nb[0] // cw - 1) * n + mr.node_geometry(nb[1])[2]) for nb in got]
            assert rel == exp, (k, s, p, rel, exp)
            tabled += 1
    assert tabled == 3 * 12 + 4       # every shape and part of the three larger CUs, 2NxN and Nx2N of the 8x8 CU


def test_second_pu_rules_follow_from_the_coding_order():
    """HM excludes L for part 1 of the vertical shapes and A for part 1 of the horizontal ones because the sample lies in part 0 of the same CU: exactly
    these, and no other candidate of any of the 508 PUs, fall inside the PU's own CU -- whose key is equal to itself, not smaller"""
    inside_own = set()
    for family, e, (k, s, p) in ALL_PUS:
        x0, y0, n = mp.node_rect(k)
        for j, (sx, sy) in enumerate(mpr.samples(*mp.pu_rect(k, s, p))):
            if x0 <= sx < x0 + n and y0 <= sy < y0 + n:
                inside_own.add((k, s, p, j))
                # ... and there it lies in part 0
                px, py, pw, ph = mp.pu_rect(k, s, 0)
                assert px <= sx < px + pw and py <= sy < py + ph
                assert mpr.candidates(192, 192, (0, 3), 4, k, s, p)[j] is None
    exp = {(k, s, 1, mg.A if s in HORIZ else mg.L) for _, _, (k, s, p) in ALL_PUS if p == 1}
    assert inside_own == exp and len(exp) == 254


def test_coding_order_decides_ar_and_bl():
    W = H = 192
    for lvl in (1, 2, 3):
        order, n = quadtree_order(lvl), 1 << lvl
        assert all(mg.z_index(x, y) == i for (x, y), i in order.items())

        def coded_before(x, y, bx, by):
            if y < 0:
                return True                       # the CTU row above, above right included
            if y >= n or x >= n:
                return False                      # the CTUs to the right and below
            if x < 0:
                return True                       # the CTU to the left, same row
            return order[(x, y)] < order[(bx, by)]

        first = mr.LEVEL_FIRST[lvl]
        seen = set()
        for by in range(n):
            for bx in range(n):
                k = first + by * n + bx
                for s in (range(6) if lvl < 3 else range(2)):
                    for p in (0, 1):
                        got = mpr.candidates(W, H, (0, 3), 4, k, s, p)
                        horiz = s in HORIZ
                        # the nodes AR and BL fall into, relative to the CU: see the table above
                        ar = (bx + 1, by - 1) if p == 0 and horiz else (bx + 1, by) if horiz else (bx, by - 1) if p == 0 else (bx + 1, by - 1)
                        bl = (bx - 1, by) if p == 0 and horiz else (bx - 1, by + 1) if horiz or p == 0 else (bx, by + 1)
                        exp = (ar != (bx, by) and coded_before(*ar, bx, by), bl != (bx, by) and coded_before(*bl, bx, by))
                        assert (got[mg.AR] is not None, got[mg.BL] is not None) == exp, (lvl, bx, by, s, p)
                        seen.add(exp)
        assert seen == {(True, True), (True, False), (False, True), (False, False)}


def test_a_band_cuts_off_the_upper_candidates():
    W, H = 200, 136
    cw = 4
    cut = kept = 0
    for c in (4, 5, 7):                         # CTU row 1; CTU 7 is the ragged last column
        for family, e, (k, s, p) in ALL_PUS:
            whole = mpr.candidates(W, H, (0, 3), c, k, s, p)
            band = mpr.candidates(W, H, (1, 3), c, k, s, p)
            for a, b in zip(whole, band):
                if a is not None and a[0] < cw:
                    assert b is None
                    cut += 1
                else:
                    assert a == b
                    kept += a is not None
    assert cut > 100 and kept > 1000
    # the picture's edges: nothing to the left of the first column, nothing above the first row, nothing from a CU that is not INSIDE
    assert mpr.candidates(W, H, (0, 3), 0, 0, 0, 0) == [None] * 5
    assert mpr.candidates(W, H, (0, 3), 1, 0, 1, 0) == [(0, 0), None, None, None, None]
    assert mpr.candidates(W, H, (0, 3), 6, 0, 0, 0)[mg.AR] is None          # the 64x64 node of CTU 3 crosses the right edge
    assert mpr.candidates(W, H, (0, 3), 6, 0, 0, 0)[mg.A] == (2, 0)


# ---- the list: a random draw ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def draw(oracle):
    pics, refined = mpr.random_draw()
    flat = np.ascontiguousarray(pics[1].astype(np.int16)).reshape(-1)
    planes = mr.Planes(pics[0], 8, mpr.DRAW_RANGE + 8)
    return refined, {f: mpr.expected(oracle, flat, 0, mpr.DRAW_W, pics[0], mpr.DRAW_W, mpr.DRAW_H, 8, mpr.DRAW_QP, refined, mpr.DRAW_RANGE, f, planes=planes)
                     for f in ("pu", "small")}


@pytest.mark.parametrize("family", ["pu", "small"])
def test_random_records_make_every_case_occur(draw, family):
    refined, exp = draw
    mpr.check_draw(refined, exp[family], family)
    e = exp[family]
    ok = e["num"] > 0
    # a PU is valid iff its CU is INSIDE: the ragged last column and row hold invalid records, and only those
    for c in range(12):
        for i, (k, s, p) in enumerate(mpr.FAMILIES[family][0]()):
            lvl, (gx, gy), _ = mpr.pu_geometry(mpr.DRAW_W, c, k, s, p)
            assert (tuple(e[c, i]) == mg.INVALID) == (not mg.inside(mpr.DRAW_W, mpr.DRAW_H, lvl, gx, gy)) == (not ok[c, i]), (c, k, s, p)
    assert (e["pad"] == 0).all() and (e["idx"][ok] < e["num"][ok]).all()
    assert ((e["src"][ok] == mg.ZERO) == (e["idx"][ok] == e["num"][ok] - 1)).sum() > 0


# ---- the distortion, pinned to the reference ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["pu", "small"])
def test_satd_at_the_references_own_vectors(oracle, family):
    """for every valid entry of the family in every case of the quarter-sample golden: the distortion of the w x h PU at the vector the reference's
    xPatternSearchFracDIF returned is the one the file holds for it"""
    checked = 0
    cov = mpr.FAMILIES[family][0]()
    for case in gold.frac_cases():
        planes = mr.Planes(case.ref.astype(np.int64), case.bd, case.R + 8)
        flat = np.ascontiguousarray(case.cur).reshape(-1)
        rec = case.records(family)
        for i, c in enumerate(case.ctus):
            for e, (k, s, p) in enumerate(cov):
                lvl, (gx, gy), (x, y, w, h) = mpr.pu_geometry(case.W, c, k, s, p)
                r = rec[i, e]
                assert (r["cost_best"] == gold.MARKER) == (not mg.inside(case.W, case.H, lvl, gx, gy))
                if r["cost_best"] != gold.MARKER:
                    assert mpr.satd_block(oracle, planes, flat, 0, case.W, x, y, w, h, (int(r["mvx"]), int(r["mvy"]))) == int(r["satd_best"]), (case, c, k, s, p)
                    checked += 1
    assert checked == gold.FRAC_COUNTS[family]


# ---- constructed pictures -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,fx,fy,mv", mc.HALF_CASES)
def test_a_half_sample_picture_merges_at_no_distortion(oracle, bd, fx, fy, mv):
    case = mc.half_sample_case(bd, fx, fy, mv)
    flat = np.ascontiguousarray(case["cur"].astype(np.int16)).reshape(-1)
    c1 = mg.bit_cost(1, mr.sqrt_lambda(oracle, mc.HALF_QP, bd))
    for family in ("pu", "small"):
        got = mpr.expected(oracle, flat, 0, mc.HALF_W, case["ref"], mc.HALF_W, mc.HALF_H, bd, mc.HALF_QP, case["refined"], 8, family, planes=case["planes"])
        merged, alone = mpr.check_half_sample(got, family, mc.HALF_W, mc.HALF_H, case["q"], c1)
        assert merged + alone == 6 * mpr.FAMILIES[family][1]        # 3 x 2 whole CTUs: every PU is valid


def test_two_motions_split_at_a_ctu_boundary(oracle):
    case = mc.two_motion_case(oracle)
    cur, ref = (p.astype(np.int64) for p in mc.pictures())
    flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
    got = mpr.expected(oracle, flat, 0, mc.W, ref, mc.W, mc.H, 8, mc.QP, case["refined"]["nodes"], mc.RANGE, "pu")
    mpr.check_two_motions(got, case["refined"]["pu"], (4 * mc.V2[0], 4 * mc.V2[1]), case["c"])
    # the selection on merge-aware costs: in CTU 2 two inherited halves cost two bits, less than the 64x64 CU's explicit vector; in CTU 1 nothing changes
    small = mpr.expected(oracle, flat, 0, mc.W, ref, mc.W, mc.H, 8, mc.QP, case["refined"]["nodes"], mc.RANGE, "small")
    r = case["refined"]
    rec, _, merged = mpr.select(r["nodes"][None], r["pu"][None], r["small"][None], got[None], small[None], mc.W, mc.H)
    plain = case["shapes"]
    assert (plain["best"][2, 0], rec["best"][0, 2, 0]) == (sr.capi.PART_2Nx2N, sr.capi.PART_2NxN)
    assert rec["cost_best"][0, 2, 0] == 2 * case["c"][1] < plain["cost_best"][2, 0] == rec["cost_2Nx2N"][0, 2, 0]
    # both parts of the horizontal shapes (p = 1, 4, 5), part 0 alone of the vertical ones (p = 2, 6, 7)
    assert merged[0, 2, 0] == sum(1 << b for b in (2, 3, 8, 9, 10, 11, 4, 12, 14))
    assert merged[0, 1, 0] == 0 and rec[0, 1, 0].tobytes() == plain[1, 0].tobytes()


# ---- the selection's one new rule ---------------------------------------------------------------------------------------------------------------------------

def _flat(value):
    """one CTU of plain cost arrays: nodes [1, 1, 85], PUs [1, 1, 124], small PUs [1, 1, 384]"""
    return tuple(np.full((1, 1, n), value, np.uint32) for n in (85, 124, 384))


def test_part_cost_is_the_smaller_one_and_markers_lose():
    W = H = 64
    nodes, pus, small = _flat(1000)
    none_p, none_s = np.full((1, 1, 124), mg.MARK, np.uint32), np.full((1, 1, 384), mg.MARK, np.uint32)
    base = sr.select(nodes, pus, small, W, H)
    # all merge costs MARK: the plain restatement, no bit anywhere; a missing small family on either side is all markers
    rec, costs, merged = mpr.select(nodes, pus, small, none_p, none_s, W, H)
    assert rec.tobytes() == base[0].tobytes() and costs.tobytes() == base[1].tobytes() and not merged.any()
    rec, costs, merged = mpr.select(nodes, pus, small, none_p, None, W, H)
    assert rec.tobytes() == base[0].tobytes() and costs.tobytes() == base[1].tobytes() and not merged.any()
    base_ns = sr.select(nodes, pus, None, W, H)
    rec, costs, merged = mpr.select(nodes, pus, None, none_p, None, W, H)
    assert rec.tobytes() == base_ns[0].tobytes() and costs.tobytes() == base_ns[1].tobytes()
    # the four combinations on part 0 of 2NxN of the root (entry 0 of the PUs; bit 2 * 1 + 0) and on part 1 of Nx2N of the last 8x8 CU (small entry 128 + 63 * 4 + 3;
    # bit 2 * 2 + 1): (refined, merge) -> the part's cost, the bit
    for k, fam, e, p, bit in ((0, "pu", 0, 1, 1 << 2), (84, "small", 128 + 63 * 4 + 3, 2, 1 << 5)):
        for r, m, cost, is_set in ((1000, 999, 999, True), (1000, 1000, 1000, False), (1000, 1001, 1000, False), (mg.MARK, 5, 5, True), (7, mg.MARK, 7, False),
                                   (mg.MARK, mg.MARK, mg.MARK, False)):
            pu2, sm2, mp2, ms2 = pus.copy(), small.copy(), none_p.copy(), none_s.copy()
            (pu2 if fam == "pu" else sm2)[0, 0, e] = r
            (mp2 if fam == "pu" else ms2)[0, 0, e] = m
            rec, costs, merged = mpr.select(nodes, pu2, sm2, mp2, ms2, W, H)
            assert costs[0, 0, k, p] == (mg.MARK if cost == mg.MARK else cost + 1000), (k, r, m)      # the other part costs 1000; an unavailable part makes the pair unavailable
            assert merged[0, 0, k] == (bit if is_set else 0) and not np.delete(merged[0, 0], k).any(), (k, r, m)
    # p = 0 stays the explicit 2Nx2N cost whatever the merge records hold, and saturation is as before
    rec, costs, merged = mpr.select(nodes, pus, small, np.zeros((1, 1, 124), np.uint32), np.zeros((1, 1, 384), np.uint32), W, H)
    assert (costs[0, 0, :, 0] == 1000).all() and (rec["cost_2Nx2N"] == 1000).all() and not (merged & 3).any() and not (merged & 0xC0).any()
    assert (merged[0, 0, :21] == 0xFF3C).all() and (merged[0, 0, 21:] == 0x003C).all()              # AMP bits only where the CU has AMP
    big = np.full((1, 1, 124), 0xFFFFFFFE, np.uint32)
    assert mpr.select(nodes, pus, small, big, none_s, W, H)[1][0, 0, 0, 1] == 2000
    assert mpr.select(nodes, np.full((1, 1, 124), mg.MARK, np.uint32), small, big, none_s, W, H)[1][0, 0, 0, 1] == sr.SATURATED


def test_merge_costs_flip_best_from_2Nx2N_to_2NxN():
    """a constructed node: the explicit 2Nx2N vector costs 900, the two halves of 2NxN 500 each with their own vectors -- 2Nx2N wins; the lower half inherits
    its vector for 350: 2NxN at 850 wins, and the upper half, whose merge cost is the larger one, keeps its refined cost"""
    W = H = 64
    nodes, pus, small = _flat(5000)
    mpus, msmall = np.full((1, 1, 124), mg.MARK, np.uint32), np.full((1, 1, 384), mg.MARK, np.uint32)
    nodes[0, 0, 0] = 900
    pus[0, 0, 0:2] = 500                       # node 0, 2NxN, parts 0 and 1
    rule = sr.capi.pu_shape_rule([0] * 4, [0] * 4, 0)
    plain = sr.select(nodes, pus, small, W, H, rule=rule)[0][0, 0, 0]
    assert (plain["best"], plain["cost_best"], plain["mask"]) == (sr.capi.PART_2Nx2N, 900, 1)
    mpus[0, 0, 0], mpus[0, 0, 1] = 650, 350
    rec, costs, merged = mpr.select(nodes, pus, small, mpus, msmall, W, H, rule=rule)
    r = rec[0, 0, 0]
    assert (r["best"], r["cost_best"], r["second"], r["cost_second"], r["cost_2Nx2N"]) == (sr.capi.PART_2NxN, 850, sr.capi.PART_2Nx2N, 900, 900)
    assert r["mask"] == 1 | 1 << sr.capi.PART_2NxN and merged[0, 0, 0] == 1 << (2 * sr.capi.PART_2NxN + 1)
    assert list(costs[0, 0, 0, :3]) == [900, 850, 10000]
    # every other node is what it was
    assert rec[0, 0, 1:].tobytes() == sr.select(nodes, pus, small, W, H, rule=rule)[0][0, 0, 1:].tobytes() and not merged[0, 0, 1:].any()
