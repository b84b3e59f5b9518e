"""The candidate lists of the three neighbour stages (fhevc_motion_amvp*, fhevc_motion_merge*, fhevc_motion_merge_pu*) against the REFERENCE's own list
functions, without a GPU and without the reference: tests/golden/ref_motion_candidates.npz holds what TComDataCU::fillMvpCand and
TComDataCU::getInterMergeCandidates returned on hand-set motion fields, what getPULeft / Above / AboveRight / BelowLeft / AboveLeft delivered, the reference's
getCost table at every QP and its vector bit counts (tests/quality/gen_motion_candidates_golden.py).  Against it stand the Python restatements the stages'
own tests compare kernels and host twins with -- motion_amvp_ref (positions, build_list, cost_table, eg), motion_merge_ref (neighbours, build_list),
motion_merge_pu_ref (candidates) -- and the host twin fhevc_motion_amvp_picture itself.  No entry is excluded: the compared counts are the file's totals.

Mutation check when this file was written: `<=` for `<` in the coding-order comparison of motion_merge_pu_ref.candidates makes the AMVP and the merge list
tests fail (an own-CU sample becomes a neighbour); the AL clause taken out of fhevc_mvp_choose makes the host-twin test fail at every QP.  The same flip
in motion_merge_ref.neighbours changes nothing: a node's five offsets never lead back to the node itself."""
import os

import numpy as np
import pytest

import motion_amvp_ref as ar
import motion_candidates_cases as cc
import motion_merge_pu_ref as mpr
import motion_merge_ref as mg
import motion_refine_ref as mr
from fasthevc_amd import capi
from oracle import oracle_py as op

ROWS = (0, cc.CH)


@pytest.fixture(scope="module")
def data():
    return cc.load()


def test_file_holds_what_the_issue_asks_for(data):
    assert os.path.getsize(cc.GOLDEN) < 1 << 20
    D = len(cc.KINDS)
    for f in cc.FAMILIES:
        assert data[f"mv_{f}"].shape == (D, cc.N, cc.PER[f], 2) and data[f"mv_{f}"].dtype == np.int16
        assert data[f"marker_{f}"].shape == (D, cc.N, cc.PER[f]) and data[f"ref_{f}"].shape == (D, cc.N, cc.PER[f], cc.REC)
        ins = cc.tables(f)[2]
        assert not data[f"ref_{f}"][:, ~ins].any()                                       # answers for INSIDE entries only
        assert not data[f"ref_{f}"][list(cc.AMVP_DRAWS)][..., cc.MERGE0:cc.COUNT + 1].any()   # an AMVP draw records the AMVP list
        assert (data[f"ref_{f}"][list(cc.MERGE_DRAWS)][:, ins][..., cc.COUNT] & 15 == 5).all()
        assert int(cc.compared(f, data[f"marker_{f}"]).sum()) == cc.COMPARED[f]
        assert int(ins.sum()) * len(cc.MERGE_DRAWS) == cc.COMPARED_MERGE[f]
        # merge draws stay within the reach of max_range 8, AMVP draws hold the int16 extremes
        assert np.abs(data[f"mv_{f}"][list(cc.MERGE_DRAWS)].astype(np.int64)).max() == 4 * cc.MERGE_RANGE + 3
        assert data[f"mv_{f}"][list(cc.AMVP_DRAWS)].max() == 32767 and data[f"mv_{f}"][list(cc.AMVP_DRAWS)].min() == -32768
    assert data["cost"].shape == (52, 67) and len(data["bit_counts"]) == len(cc.bit_pairs()) and np.array_equal(data["bit_pairs"], cc.bit_pairs())
    seen = cc.coverage(data)
    for f in cc.FAMILIES:
        for lvl in ar.LEVELS[f]:
            got = tuple(seen[("amvp", f, lvl, name)] for name in cc.NAMES)
            assert got == cc.SUPPLIED[(f, lvl)], (f, lvl, got)
            for name, n in zip(cc.NAMES, got):
                if ("amvp", f, lvl, name) in cc.EXCUSED:
                    assert n == 0, (f, lvl, name, n)                                       # the reference itself reports none
                else:
                    assert n >= cc.required(f, lvl), (f, lvl, name, n)
    assert all(k[0] == "amvp" and k[1] in cc.FAMILIES and k[3] in cc.NAMES for k in cc.EXCUSED)
    assert {s: seen[("own", s)] for s in cc.SHAPES} == cc.OWN and min(cc.OWN.values()) >= cc.MIN_SUPPLIED
    assert {n: seen[("merge_length", n)] for n in range(1, 6)} == cc.MERGE_LENGTHS and min(cc.MERGE_LENGTHS.values()) >= cc.MIN_SUPPLIED
    assert {p: seen[("pair",) + p] for p in cc.PAIRS} == cc.PAIRS and min(cc.PAIRS.values()) >= cc.MIN_SUPPLIED
    assert seen[("al_dropped",)] == cc.AL_DROPPED >= cc.MIN_SUPPLIED and seen[("amvp_prune",)] == cc.AMVP_PRUNED >= cc.MIN_SUPPLIED


def candidates_of(pos, e, p0, mv, marker):
    """positions() of one entry -> the five (x, y) or None, as build_list takes them: a same-level node from the nodes' inputs, "own" from part 0 of the
    entry's own family"""
    out = []
    for where in pos:
        if where is None:
            out.append(None)
        elif where[0] == "own":
            out.append(None if marker["own"][p0[e]] else tuple(int(v) for v in mv["own"][p0[e]]))
        else:
            c, k = where[1], where[2]
            out.append(None if marker["nodes"][c, k] else tuple(int(v) for v in mv["nodes"][c, k]))
    return out


def test_amvp_list_and_positions_equal_the_reference(data):
    """motion_amvp_ref.positions + build_list against fillMvpCand's two candidates, and every position's availability, vector and own-CU flag against the
    reference's five neighbour functions, on every INSIDE entry that is no marker"""
    for f in cc.FAMILIES:
        plan = ar.plan(cc.W, cc.H, ROWS, f)
        p0 = cc.tables(f)[3]
        n = 0
        for d in range(len(cc.KINDS)):
            mv, marker, ref = cc.draw(data, d)
            found, own, vec = cc.flags(ref[f])
            for c, e in np.argwhere(cc.compared(f, marker[f])):
                pos = plan[c][e]
                assert pos is not None
                cands = candidates_of(pos, e, p0, dict(nodes=mv["nodes"], own=mv[f][c]), dict(nodes=marker["nodes"], own=marker[f][c]))
                for j in range(5):
                    what = (f, d, int(c), int(e), cc.NAMES[j])
                    assert (cands[j] is not None) == bool(found[c, e, j]), what
                    assert (pos[j] is not None and pos[j][0] == "own") == bool(own[c, e, j]), what
                    if cands[j] is not None:
                        assert cands[j] == tuple(vec[c, e, j]), what
                        if own[c, e, j]:
                            assert cands[j] == tuple(mv[f][c, p0[e]]), what                   # the reference delivers part 0's vector
                lst, _ = ar.build_list(cands)
                assert [tuple(int(v) for v in ref[f][c, e, 2 * i:2 * i + 2]) for i in range(2)] == [v for _, v in lst], (f, d, int(c), int(e), cands)
                n += 1
        assert n == cc.COMPARED[f]


def test_merge_lists_equal_the_reference(data):
    """motion_merge_ref.neighbours / motion_merge_pu_ref.candidates + motion_merge_ref.build_list at max_range 8 against getInterMergeCandidates on every
    INSIDE entry of the merge draws: equal up to the restatement's own length, whose last entry is the first filled zero; behind it zero vectors; refIdx 0
    and direction 1 throughout; five candidates"""
    for f in cc.FAMILIES:
        cov, _, ins, _ = cc.tables(f)
        n = 0
        for d in cc.MERGE_DRAWS:
            mv, marker, ref = cc.draw(data, d)
            lists, rest, count, spatial = cc.merge_list(ref[f])
            for c, e in np.argwhere(ins):
                k, s, p = cov[e]
                if s is None:
                    lvl, bx, by = mr.node_geometry(k)
                    nbs = mg.neighbours(cc.W, cc.H, ROWS, lvl, (c % cc.CW) * (1 << lvl) + bx, (c // cc.CW) * (1 << lvl) + by)
                else:
                    nbs = mpr.candidates(cc.W, cc.H, ROWS, c, k, s, p)
                cands = [None if nb is None else ((cc.MARK if marker["nodes"][nb] else 0),) + tuple(int(v) for v in mv["nodes"][nb]) for nb in nbs]
                lst = mg.build_list(cands, cc.MERGE_RANGE)
                what = (f, d, int(c), int(e), cands, ref[f][c, e].tolist())
                assert [v for _, v in lst] == [tuple(int(x) for x in v) for v in lists[c, e, :len(lst)]], what
                assert lst[-1][0] == mg.ZERO and len(lst) == spatial[c, e] + 1, what
                assert not lists[c, e, len(lst):].any() and (rest[c, e] == (1, 0)).all() and count[c, e] == 5, what
                n += 1
        assert n == cc.COMPARED_MERGE[f]


def test_cost_table_and_bit_counts_equal_the_reference(data):
    for qp in range(52):
        assert ar.cost_table(qp) == data["cost"][qp].tolist(), qp
    assert len(ar.cost_table(0)) == ar.BIT_COSTS == 67
    pairs, counts = data["bit_pairs"], data["bit_counts"]
    assert {int(v) for v in pairs[:, 0] - pairs[:, 2]} >= set(cc.DIFFS) and {int(v) for v in pairs[:, 1] - pairs[:, 3]} >= set(cc.DIFFS)
    for (vx, vy, px, py), bits in zip(pairs.tolist(), counts.tolist()):
        assert ar.eg(vx - px) + ar.eg(vy - py) == bits, (vx, vy, px, py)
    assert counts.max() == 66 and counts.min() == 2
    d = np.arange(-70000, 70001)
    assert cc.eg_array(d).tolist() == [ar.eg(int(v)) for v in d]                           # the vectorised form the kernel checks use


@pytest.mark.parametrize("qp", [0, ar.DRAW_QP, 51])
def test_host_twin_prices_on_the_references_candidates(data, qp):
    """fhevc_motion_amvp_picture on every draw: predictor, index and bits are the first index of least bits over the reference's two candidates, the cost is
    min(satd_best + the reference's getCost[bits], 0xFFFFFFFE); nothing of motion_amvp_ref.expected is involved"""
    rng = np.random.default_rng(99)
    ones, high = dict.fromkeys(cc.FAMILIES, 0), set()
    for d in range(len(cc.KINDS)):
        mv, marker, ref = cc.draw(data, d)
        rec = {f: cc.records(rng, mv[f], marker[f]) for f in cc.FAMILIES}
        got = capi.motion_amvp_picture(rec["nodes"], rec["pu"], rec["small"], cc.W, cc.H, qp=qp, with_mvp=True)
        for i, f in enumerate(cc.FAMILIES):
            won, bits = cc.check_amvp(f, rec[f], ref[f], data["cost"][qp], got[i], got[3 + i], (d, qp))
            ones[f] += won
            high |= set(bits[bits >= 39].tolist())
    assert min(ones.values()) >= 8, ones                                                   # both list slots are seen through the host twin
    assert len(high) >= 8 and max(high) == 66, sorted(high)                                # table entries above 38 against the reference's numbers


@pytest.mark.skipif(not op.have_candidates(), reason="oracle/_ref not built from this tree's harness (no reference sources here; make -C oracle ref)")
def test_the_reference_still_gives_the_file(data):
    """one draw of each kind and both tables through oracle/_ref's library"""
    lib = op.bind_candidates(op.load_ref())
    for d in (cc.AMVP_DRAWS[0], cc.MERGE_DRAWS[-1]):
        mv, marker, ref = cc.draw(data, d)
        again = cc.record(lib, mv, marker, cc.KINDS[d] == "merge")
        for f in cc.FAMILIES:
            assert np.array_equal(again[f], ref[f]), (d, f)
    cost, bits = cc.tables_from(lib)
    assert np.array_equal(cost, data["cost"]) and np.array_equal(bits, data["bit_counts"])
