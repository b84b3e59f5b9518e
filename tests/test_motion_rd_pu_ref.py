"""The restatement of the RD stage under a partition size (tests/motion_rd_pu_ref.py) without a GPU: 2Nx2N is motion_rd_ref's record, the kernel's
quadrant -> part arithmetic agrees with getPartIndexAndSize for every (node, size, quadrant), closed forms on pictures built by the interpolation
filter itself, the merged rule, the three sources of side bits, the fold's five outcomes -- and what the draw of tests/test_gpu_motion_rd_pu.py holds,
asserted here on the inputs alone."""
import numpy as np
import pytest

import motion_pu_ref as mp
import motion_rd_pu_ref as pu
import motion_rd_ref as rd
import motion_refine_ref as mr
from fasthevc_amd import capi

QDT, MDT, PDT = capi.MOTION_QPEL_DTYPE, capi.MOTION_MERGE_DTYPE, capi.MOTION_MVP_DTYPE
_CACHE = {}


def draw(bd=8):
    if bd not in _CACHE:
        ref, cur = rd.draw_pictures(bd)
        _CACHE[bd] = (ref, cur, mr.Planes(ref, bd, 16))
    return _CACHE[bd]


def test_2Nx2N_is_the_rd_stage_on_bytes_0_to_11():
    ref, cur, planes = draw()
    for with_mvp in (False, True):
        inp = pu.draw_inputs(11, 8, with_mvp=with_mvp)[0]
        got = pu.expected(cur, ref, pu.W, pu.H, 8, 27, 0, inp, 8, planes=planes)
        base = rd.expected(cur, ref, pu.W, pu.H, 8, 27, inp.nodes, rd.EXPLICIT, 8, mvp=inp.mvp_nodes, planes=planes)
        assert np.array_equal(got.view(np.uint8).reshape(-1, 16)[:, :12], base.view(np.uint8).reshape(-1, 16)[:, :12])
        ok = base["cost_rd"] != rd.MARK
        assert ok.sum() > 200 and (got["part"][ok] == 0).all() and (got["part"][~ok] == 255).all() and not got["merged"].any() and not got["pad"].any()


def test_kernel_quadrant_arithmetic_agrees_with_pu_rect():
    """every tile of every node, every size that node has, every 4x4 quadrant: the part by the kernel's arithmetic is the part whose rectangle holds it"""
    checked = straddling = 0
    for k in range(85):
        lvl, bx, by = mr.node_geometry(k)
        t = max((64 >> lvl) // 8, 1)
        for p in pu.TWO_PART:
            if pu.sr.parts(k, p) is None:
                continue
            rects = [mp.pu_rect(k, pu.sr.shape_of(p), part) for part in (0, 1)]
            for ty in range(by * t, by * t + t):
                for tx in range(bx * t, bx * t + t):
                    for q in range(4):
                        x, y = tx * 8 + (q & 1) * 4, ty * 8 + (q >> 1) * 4
                        holds = [r[0] <= x and x + 4 <= r[0] + r[2] and r[1] <= y and y + 4 <= r[1] + r[3] for r in rects]
                        assert sum(holds) == 1 and holds[pu.kernel_quadrant_part(lvl, tx, ty, p, q)], (k, p, tx, ty, q)
                        checked += 1
                    s = pu.straddles(lvl, tx, ty, p)
                    assert not s or lvl == 3 or (lvl == 2 and p >= 4), (k, p)        # only AMP of the 16x16 nodes and the 8x8 nodes cut a tile
                    straddling += s
    assert checked == 4 * (64 * 6 * 2 + 64 * 6 + 64 * 2) and straddling == 16 * 4 * 2 + 64 * 2


QA, QB = (5, 2), (-6, 7)


def constructed(bd=8):
    """the ten constructed CTUs, one per kind: (reference, current, planes)"""
    key = ("two", bd)
    if key not in _CACHE:
        rng = np.random.default_rng(3 + bd)
        yy, xx = np.mgrid[0:64, 0:640].astype(np.float64)
        top = (1 << bd) - 1
        ref = np.clip((0.5 + 0.2 * np.sin(xx / 7.0) * np.cos(yy / 5.0)) * top + rng.normal(0, 0.08 * top, size=xx.shape), 0, top).astype(np.int64)
        planes = mr.Planes(ref, bd, 16)
        _CACHE[key] = (ref, pu.two_motion_picture(planes, pu.KIND_ORDER, QA, QB), planes)
    return _CACHE[key]


@pytest.mark.parametrize("bd,qp", [(8, 27), (10, 37)])
def test_closed_forms_on_pictures_built_by_the_filter(bd, qp):
    ref, cur, planes = constructed(bd)
    n = len(pu.KIND_ORDER)
    lam = rd.lam_q8(qp)
    inp = pu.two_motion_inputs(pu.KIND_ORDER, QA, QB)
    at_b = inp._replace(nodes=pu.two_motion_inputs(pu.KIND_ORDER, QB, QA).nodes)
    whole = [pu.expected(cur, ref, 64 * n, 64, bd, qp, 0, x, 8, planes=planes) for x in (inp, at_b)]
    side = mr.eg_bits(QA[0]) + mr.eg_bits(QA[1]) + mr.eg_bits(QB[0]) + mr.eg_bits(QB[1])     # no predictor records: both parts against zero
    for i, kind in enumerate(pu.KIND_ORDER):
        p = pu.part_size_of_kind(kind)
        two = pu.expected(cur, ref, 64 * n, 64, bd, qp, p, inp, 8, planes=planes)
        for k in pu.TWO_MOTION_KINDS[kind][2]:
            r = two[i, k]
            tus = 4 if k == 0 else 1
            assert r["dist"] == 0 and r["flags"] & 1 and r["part"] == p and r["merged"] == 0 and r["tu_split"] == 0, (kind, k, r)
            assert r["bits"] == side + 2 * tus and r["cost_rd"] == (lam * int(r["bits"])) >> 8, (kind, k, r)
            assert whole[0][i, k]["dist"] > 0 and whole[1][i, k]["dist"] > 0, (kind, k)     # one vector cannot predict two motions
            for first in whole:
                assert pu.fold(two[i:i + 1, k], first[i:i + 1, k])[0]["part"] == p and pu.fold(first[i:i + 1, k], two[i:i + 1, k])[0]["part"] == p, (kind, k)


def _q(cost, v=(1, 2)):
    return np.array([(0, 0, cost, v[0], v[1])], QDT)[0]


def _m(cost, v=(3, -4), idx=2):
    return np.array([(0, cost, v[0], v[1], idx, 5, 0, 0)], MDT)[0]


def test_the_merged_rule_and_the_side_bits():
    reach = 35
    eg = lambda v: mr.eg_bits(v[0]) + mr.eg_bits(v[1])
    # one less / equal / one more: strictly smaller only
    assert pu.part_choice(_q(100), _m(99), None, reach) == (True, (3, -4), 3, True)
    assert pu.part_choice(_q(100), _m(100), None, reach) == (True, (1, 2), eg((1, 2)), False)
    assert pu.part_choice(_q(100), _m(101), None, reach) == (True, (1, 2), eg((1, 2)), False)
    # both markers, one marker either way
    assert not pu.part_choice(_q(pu.MARK), _m(pu.MARK), None, reach)[0] and not pu.part_choice(_q(pu.MARK), None, None, reach)[0]
    assert pu.part_choice(_q(pu.MARK), _m(7), None, reach) == (True, (3, -4), 3, True)
    assert pu.part_choice(_q(7), _m(pu.MARK), None, reach) == (True, (1, 2), eg((1, 2)), False)
    # the three sources of side bits: the merge index (4 saves its last bit), the predictor record, the exp-Golomb lengths against zero
    assert [pu.part_choice(_q(9), _m(1, idx=i), None, reach)[2] for i in range(5)] == [1, 2, 3, 4, 4]
    v = np.array([(0, 0, 1, 2, 0, 17)], PDT)[0]
    assert pu.part_choice(_q(9), _m(9), v, reach) == (True, (1, 2), 17, False)
    v["idx"] = 255
    assert not pu.part_choice(_q(9), _m(9), v, reach)[0] and pu.part_choice(_q(9), _m(8), v, reach)[0]     # a merged part does not ask its predictor record
    assert pu.part_choice(_q(9, (-5, 0)), None, None, reach)[2] == mr.eg_bits(-5) + mr.eg_bits(0) == 8
    # the reach, per component, of the vector that was chosen
    assert pu.part_choice(_q(9, (35, -35)), None, None, reach)[0] and not pu.part_choice(_q(9, (36, 0)), None, None, reach)[0]
    assert not pu.part_choice(_q(9), _m(8, (0, -36)), None, reach)[0] and pu.part_choice(_q(9, (36, 0)), _m(8), None, reach)[0]


def test_the_folds_five_outcomes():
    new, old = pu.marker((5,)), pu.marker((5,))
    for i, (n, o) in enumerate(((10, 11), (11, 10), (10, 10), (10, None), (None, 10))):
        if n is not None:
            new[i] = (1, n, 2, 0, 0, 1, 1, (0, 0))
        if o is not None:
            old[i] = (3, o, 4, 1, 0, 0, 0, (0, 0))
    out = pu.fold(new, old)
    assert out["part"].tolist() == [1, 0, 0, 1, 0] and out["dist"].tolist() == [1, 3, 3, 1, 3]
    assert pu.fold_outcome(new, old).tolist() == [0, 1, 2, 3, 4]
    both = pu.fold(pu.marker((2,)), pu.marker((2,)))
    assert both.tobytes() == pu.marker((2,)).tobytes()


def test_what_the_draw_holds():
    """conditions on the inputs of tests/test_gpu_motion_rd_pu.py's main draw (seed, ranges and number of pairs are that file's)"""
    for max_range in (8, 64):
        draws = pu.draw_inputs(pu.MAIN_SEED, max_range, nf=pu.MAIN_PAIRS + 1)
        different, merged, straddling = {}, {l: [0, 0] for l in range(4)}, {l: 0 for l in range(4)}
        reach = 4 * max_range + 3
        for inp in draws:
            st = pu.draw_statistics(inp, max_range)
            for l in range(4):
                merged[l][0] += st["merged"][l][0]
                merged[l][1] += st["merged"][l][1]
                straddling[l] += st["straddling"][l]
            for i in range(pu.N):
                for k in range(85):
                    lvl, bx, by = mr.node_geometry(k)
                    n = 64 >> lvl
                    if (i % pu.CW) * 64 + (bx + 1) * n > pu.W or (i // pu.CW) * 64 + (by + 1) * n > pu.H:
                        continue
                    for p in pu.TWO_PART:
                        got = pu.node_choice(inp, i, k, p, reach)
                        if got is not None and got[1][0] != got[1][1]:
                            different[(lvl, p)] = different.get((lvl, p), 0) + 1
        for lvl in range(4):
            for p in pu.TWO_PART:
                if lvl == 3 and p >= 4:
                    assert (lvl, p) not in different
                else:
                    assert different.get((lvl, p), 0) >= 8, (max_range, lvl, p, different)
            assert merged[lvl][0] >= 8 and merged[lvl][1] >= 8, (max_range, lvl, merged)
        assert straddling[2] >= 8 and straddling[3] >= 8 and straddling[0] == straddling[1] == 0, straddling


def test_the_draw_holds_every_fold_outcome():
    ref, cur, planes = draw()
    inp = pu.draw_inputs(pu.MAIN_SEED, 8, nf=2)[0]
    first = pu.expected(cur, ref, pu.W, pu.H, 8, 27, 0, inp, 8, planes=planes)
    counts = np.zeros(5, np.int64)
    acc = first
    for mode in (pu.BEST, pu.SECOND):
        new = pu.expected(cur, ref, pu.W, pu.H, 8, 27, mode, inp, 8, planes=planes)
        counts += np.bincount(pu.fold_outcome(new, acc).ravel(), minlength=5)
        acc = pu.fold(new, acc)
    counts += np.bincount(pu.fold_outcome(acc, acc).ravel(), minlength=5)          # the tie: a launch folded with itself
    assert (counts >= 8).all(), counts
    assert pu.fold(acc, acc).tobytes() == acc.tobytes()
    # the three-launch sequence is the chain of the frame call
    merge_nodes, _ = rd.draw_records(rd.MERGE, 5, 8)
    _, rd_pu, dmin, dmax = pu.frame_records(cur, ref, pu.W, pu.H, 8, 27, 8, inp, merge_nodes, 3, planes=planes)
    assert rd_pu.tobytes() == acc.tobytes() and dmin.shape == (pu.N, 256) and (dmin <= dmax).all()
    assert set(np.unique(acc["part"])) >= {0, 1, 2, 4, 5, 6, 7, 255}
