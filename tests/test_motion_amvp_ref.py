"""The Python restatement of the re-pricing against neighbour predictors (tests/motion_amvp_ref.py) held to hand-written expectations and to the
reference's recorded costs, without a GPU: the list rules by enumeration, the own-CU candidate of every part 1, the closed form of a uniform pan, a pin
to tests/golden/ref_frac_search*.npz (re-pricing is translation invariant: a record the reference priced against zero, presented as q + p with the single
neighbour p, must come out at the reference's own cost), and the conditions on the random draw the other two test files rest on."""
import itertools

import numpy as np

import motion_amvp_ref as ar
import motion_golden
import motion_merge_ref as mg
import motion_refine_ref as mr
import motion_refine_wide_cases

L, A, AR, BL, AL, ZERO = ar.L, ar.A, ar.AR, ar.BL, ar.AL, ar.ZERO


def test_motion_lambda_is_the_oracles_at_every_qp_and_bit_depth(oracle):
    for qp in range(52):
        for bd in (8, 10, 12):
            assert ar.sqrt_lambda(qp) == mr.sqrt_lambda(oracle, qp, bd)
    assert ar.cost_table(32)[2] == mg.bit_cost(2, ar.sqrt_lambda(32)) and len(ar.cost_table(0)) == 67


def test_eg_by_hand():
    # t = 1 | 2, 3 | 4..7 | 8..15 ...: 0 -> 1 bit, +-1 -> 3, +-2, +-3 -> 5 (t = 4, 5 / 6, 7), 4 -> 7 (t = 8), -4 -> 7 (t = 9)
    assert [ar.eg(v) for v in (0, 1, -1, 2, -2, 3, -3, 4, -4, 7, -7, 8)] == [1, 3, 3, 5, 5, 5, 5, 7, 7, 7, 7, 9]
    assert ar.eg(32767) == 31 and ar.eg(-32767) == 31 and ar.eg(32768) == 33 and ar.eg(-32768) == 33 and ar.eg(65535) == 33 and ar.eg(-65535) == 33


def test_list_rules_by_enumeration():
    vec = {L: (11, -1), A: (12, -2), AR: (13, -3), BL: (14, -4), AL: (15, -5)}
    for mask in itertools.product((False, True), repeat=5):
        cands = [vec[j] if mask[j] else None for j in range(5)]
        lst, n = ar.build_list(cands)
        # written out by hand: BL before L; AR before A before AL
        left = BL if mask[BL] else (L if mask[L] else None)
        above = AR if mask[AR] else (A if mask[A] else (AL if mask[AL] else None))
        want = [(j, vec[j]) for j in (left, above) if j is not None]
        assert n == len(want) and lst == want + [(ZERO, (0, 0))] * (2 - len(want)), (mask, lst)
    # every fallback order, spelled out
    assert ar.build_list([vec[L], None, None, None, None])[0] == [(L, vec[L]), (ZERO, (0, 0))]
    assert ar.build_list([vec[L], None, None, vec[BL], None])[0][0] == (BL, vec[BL])
    assert ar.build_list([None, vec[A], None, None, vec[AL]])[0][0] == (A, vec[A])
    assert ar.build_list([None, None, None, None, vec[AL]])[0] == [(AL, vec[AL]), (ZERO, (0, 0))]
    assert ar.build_list([None, vec[A], vec[AR], None, vec[AL]])[0][0] == (AR, vec[AR])
    # dedupe: the second of two equal entries goes, and a zero comes in its place; equal vectors on one side never meet
    same = (7, 7)
    assert ar.build_list([same, same, None, None, None]) == ([(L, same), (ZERO, (0, 0))], 1)
    assert ar.build_list([None, None, same, same, None]) == ([(BL, same), (ZERO, (0, 0))], 1)
    assert ar.build_list([same, (1, 1), None, same, None]) == ([(BL, same), (A, (1, 1))], 2)
    assert ar.build_list([(0, 0), (0, 0), None, None, None]) == ([(L, (0, 0)), (ZERO, (0, 0))], 1)       # a spatial zero is deduped like any vector
    # zero fill at 0, 1 and 2 spatial entries
    assert ar.build_list([None] * 5) == ([(ZERO, (0, 0)), (ZERO, (0, 0))], 0)
    assert ar.build_list([None, (3, 4), None, None, None]) == ([(A, (3, 4)), (ZERO, (0, 0))], 1)
    assert ar.build_list([(1, 2), (3, 4), None, None, None]) == ([(L, (1, 2)), (A, (3, 4))], 2)
    # the choice: index 1 wins only with strictly fewer bits
    lst = [(L, (40, 40)), (A, (3, 3))]
    assert ar.choose((3, 3), lst) == (1, [ar.eg(-37) * 2, 2])
    assert ar.choose((40, 40), lst) == (0, [2, ar.eg(37) * 2])
    assert ar.choose((2, 2), [(L, (4, 4)), (ZERO, (0, 0))]) == (0, [10, 10])                              # a tie goes to index 0
    assert ar.choose((0, 0), [(ZERO, (0, 0)), (ZERO, (0, 0))]) == (0, [2, 2])


def test_own_cu_candidate_of_every_part_1():
    """on CTU 3 of a 128 x 128 picture (every neighbour exists): the only positions that fall into the entry's own CU are L of part 1 of Nx2N / nLx2N /
    nRx2N (shapes 1, 4, 5) and A of part 1 of 2NxN / 2NxnU / 2NxnD (shapes 0, 2, 3)"""
    count = 0
    for family in ("pu", "small"):
        for k, s, p in ar.covered(family):
            pos = ar.positions(128, 128, (0, 2), 3, k, s, p)
            own = [j for j, w in enumerate(pos) if w is not None and w[0] == "own"]
            want = [] if p == 0 else ([L] if s in (1, 4, 5) else [A])
            assert own == want, (family, k, s, p, pos)
            count += 1
    assert count == 508
    for k in range(85):
        assert all(w is None or w[0] == "node" for w in ar.positions(128, 128, (0, 2), 3, k, None, 0))


def test_uniform_pan_closed_form():
    """every record carries q, none is a marker: an entry with any available candidate is priced against q itself (2 bits), one without against zero"""
    W, H, qp, q = ar.DRAW_W, ar.DRAW_H, 27, (76, -3)
    c = ar.cost_table(qp)
    rng = np.random.default_rng(3)
    ins = {}
    for f, per in ar.PER.items():
        a = np.zeros((9, per), ar.QDT)
        a["satd_int"], a["satd_best"], a["cost_best"] = rng.integers(0, 90000, (9, per)), rng.integers(0, 90000, (9, per)), rng.integers(0, 90000, (9, per))
        a["mvx"], a["mvy"] = q
        ins[f] = a
    exp = ar.expected_all(W, H, ins["nodes"], ins["pu"], ins["small"], qp)
    with_c = without = 0
    for f in ar.PER:
        rec, mvp = exp[f]
        for i, per_ctu in enumerate(ar.plan(W, H, (0, 3), f)):
            for e, pos in enumerate(per_ctu):
                if pos is None:
                    assert tuple(rec[i, e]) == ar.MARKER
                    continue
                has = any(w is not None for w in pos)
                bits = 2 if has else ar.eg(q[0]) + ar.eg(q[1])
                assert rec["cost_best"][i, e] == ins[f]["satd_best"][i, e] + c[bits], (f, i, e)
                assert (rec["satd_int"][i, e], rec["satd_best"][i, e], rec["mvx"][i, e], rec["mvy"][i, e]) == (ins[f]["satd_int"][i, e], ins[f]["satd_best"][i, e], q[0], q[1])
                assert mvp["bits"][i, e] == bits and (mvp["px"][i, e], mvp["py"][i, e]) == (q if has else (0, 0))
                with_c, without = with_c + has, without + (not has)
    assert with_c > 3000 and without >= 3           # the first CU of the picture has no neighbour, at every level and in every family


def test_reference_costs_are_reproduced_under_any_translation():
    """Re-pricing is translation invariant.  Every valid record (q, satd_best, cost_best) of the two quarter-sample goldens, priced by the reference against
    zero, is presented as the vector q + p with the single available neighbour p: it must come out at the reference's own cost_best.  This pins eg and
    c[b] up to the 38 bits those files reach; entries 39..66 of the table rest on the formula"""
    # the files' vectors stay within +-259 quarter samples: beyond |p| = 518 per component the zero fill can never take fewer bits than p (eg grows with |v|),
    # so the neighbour is the predictor and the price is that of q against zero
    shifts = ((0, 0), (600, -600), (-1000, 777), (32000, -32000), (-32000, 32000), (-32000, -32000))
    compared, top = 0, 0
    for case in motion_golden.frac_cases() + motion_refine_wide_cases.wide_frac_cases():
        c = ar.cost_table(case.qp)
        for family in ("nodes", "pu", "small"):
            r = case.records(family)
            r = r[r["cost_best"] != ar.MARK]
            for qx, qy, satd, cost in zip(r["mvx"].tolist(), r["mvy"].tolist(), r["satd_best"].tolist(), r["cost_best"].tolist()):
                for p in shifts:
                    lst, n = ar.build_list([p, None, None, None, None])
                    idx, bits = ar.choose((qx + p[0], qy + p[1]), lst)
                    if p != (0, 0):
                        assert (n, lst[0]) == (1, (L, p))
                        assert idx == 0 and abs(qx) <= 259 and abs(qy) <= 259
                    assert satd + c[bits[idx]] == cost, (case, family, qx, qy, p)
                    top = max(top, bits[idx])
                compared += 1
    assert compared == sum(motion_golden.FRAC_COUNTS.values()) + sum(motion_refine_wide_cases.WIDE_FRAC_COUNTS.values())
    assert top == 38


def test_the_draw_shows_every_outcome():
    """per family at least 8 entries of every applicable outcome; on the 64x64 level (four nodes of the picture) each applicable outcome at least once
    over the draws -- BL of a 64x64 NODE lies in a CTU that follows in coding order, so src 3 cannot occur there"""
    ins, exp, stats = ar.draw_batch()
    assert ins["nodes"].shape == (ar.DRAWS, 9, 85) and 0.05 < (ins["small"]["cost_best"] == ar.MARK).mean() < 0.15
    for family in ar.PER:
        assert set(stats[family]) == set(ar.LEVELS[family])
        total = sum(stats[family].values(), ar.collections.Counter())
        for o in ar.APPLICABLE[family]:
            assert total[o] >= 8, (family, o, total[o])
        if 0 in stats[family]:
            for o in ar.APPLICABLE[family]:
                if not (family == "nodes" and o == "src_3"):
                    assert stats[family][0][o] >= 1, (family, o)
        rec, mvp = exp[family]
        priced = mvp["idx"] != 255
        assert (rec["cost_best"][priced] != ar.MARK).all() and (rec["cost_best"][priced] == ar.SAT).any()
        assert (mvp["bits"][priced] >= 2).all() and mvp["bits"].max() <= 66 and mvp["bits"][priced].max() >= 62
    assert stats["nodes"][0]["src_3"] == 0
