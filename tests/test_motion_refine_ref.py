"""Pins tests/motion_refine_ref.py, the numpy restatement the quarter-sample refinement kernel is held to (no GPU needed): the interpolation
paths agree where they must, the vector cost is the oracle's at integer positions, the order of the two candidate tables decides ties, and a
picture made by the filter itself at a half-sample offset is found exactly, with zero distortion, on every node."""
import numpy as np
import pytest

import motion_refine_ref as mr
from fasthevc_amd import frames


def textured(W, H, bd, seed):
    """noise over a smooth base, full range of bd bits"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.3 * np.sin(xx / 11.0) * np.cos(yy / 7.0)
    v = base * ((1 << bd) - 1) + rng.normal(0, 40 << (bd - 8), size=(H, W))
    return np.clip(np.rint(v), 0, (1 << bd) - 1).astype(np.int64)


def flat_plane(pic):
    """[H, W] samples -> (flat int16, origin, stride) without margins"""
    a = np.ascontiguousarray(pic.astype(np.int16))
    return a.reshape(-1), 0, a.shape[1]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_interpolation_paths_agree(bd):
    p = textured(96, 80, bd, 3 + bd)
    p[:8, :8] = 0
    p[8:16, :8] = (1 << bd) - 1     # full swing: the clip is exercised
    inner = (slice(3, -4), slice(3, -4))
    assert np.array_equal(mr.interpolate(p, 0, 0, bd), p)
    assert mr.TAPS[3] == mr.TAPS[1][::-1] and all(sum(c) == 64 for c in mr.TAPS.values())
    for f in (1, 2, 3):
        # vertical only: through the 14-bit intermediate and directly
        assert np.array_equal(mr.vertical_through_intermediate(p, f, bd)[inner], mr.interpolate(p, 0, f, bd)[inner])
        # the vertical filter is the horizontal one on the transposed picture
        assert np.array_equal(mr.interpolate(p, 0, f, bd)[inner], mr.interpolate(p.T.copy(), f, 0, bd).T[inner])
        # c3 mirrors c1, c2 itself: filtering the mirrored picture at f equals the mirror of filtering at 4 - f, one sample further
        a = mr.interpolate(p[:, ::-1].copy(), f, 0, bd)[:, ::-1]
        b = mr.interpolate(p, 4 - f, 0, bd)
        assert np.array_equal(a[:, 5:-5], b[:, 4:-6])
    # a constant picture stays constant in all sixteen planes
    k = np.full((40, 40), 77 << (bd - 8), np.int64)
    for fy in range(4):
        for fx in range(4):
            assert (mr.interpolate(k, fx, fy, bd)[inner] == k[0, 0]).all(), (fx, fy)
    # the two-stage form is not the product of two rounded one-stage passes: the planes do differ somewhere, and the both-fractional one is in range
    d = mr.interpolate(p, 2, 2, bd)
    assert d.min() >= 0 and d.max() <= (1 << bd) - 1 and not np.array_equal(d, mr.interpolate(mr.interpolate(p, 2, 0, bd), 0, 2, bd))


def test_vector_cost_is_the_oracles_at_integer_positions(oracle):
    for qp in (0, 22, 37, 51):
        sl = mr.sqrt_lambda(oracle, qp, 8)
        for mx in (-64, -9, -1, 0, 1, 2, 7, 33, 64):
            for my in (-64, -3, 0, 5, 64):
                assert mr.qpel_cost(4 * mx, 4 * my, sl) == oracle.fho_mv_cost(mx, my, sl)
    assert max(mr.eg_bits(q) for q in range(-259, 260)) * 2 == 38
    assert [mr.eg_bits(v) for v in (0, 1, -1, 2, -2, 3, 4)] == [1, 3, 3, 5, 5, 5, 7]


@pytest.mark.parametrize("bd,qp", [(8, 22), (10, 32), (12, 37), (8, 0), (8, 51)])
def test_integer_candidate_and_final_cost(oracle, bd, qp):
    W, H = 128, 128
    ref, cur = textured(W, H, bd, 11), textured(W, H, bd, 12)
    planes = mr.Planes(ref, bd, 16)
    flat, org, stride = flat_plane(cur)
    sl = mr.sqrt_lambda(oracle, qp, bd)
    rng = np.random.default_rng(qp)
    pad = np.pad(ref, 16, mode="edge").astype(np.int16)
    for n, x0, y0 in ((64, 0, 0), (64, 64, 64), (32, 96, 0), (16, 112, 112), (8, 0, 120), (8, 56, 64)):
        mx, my = (int(v) for v in rng.integers(-8, 9, size=2))
        r = mr.refine_node(oracle, planes, flat, org, stride, x0, y0, n, mx, my, sl)
        blk = np.ascontiguousarray(pad[16 + y0 + my:16 + y0 + my + n, 16 + x0 + mx:16 + x0 + mx + n])
        o = np.ascontiguousarray(cur[y0:y0 + n, x0:x0 + n].astype(np.int16))
        satd = oracle.fho_satd(o.ctypes.data, n, blk.ctypes.data, n, n, n, bd)
        assert r["satd_int"] == satd and r["half"][0][3] == satd + oracle.fho_mv_cost(mx, my, sl)
        assert r["cost_best"] <= r["half"][0][3]
        assert r["cost_best"] == r["satd_best"] + mr.qpel_cost(r["mvx"], r["mvy"], sl)
        assert abs(r["mvx"] - 4 * mx) <= 3 and abs(r["mvy"] - 4 * my) <= 3
        # the quarter stage's centre is the half stage's winner, at the same cost
        assert r["quarter"][0] == min(r["half"], key=lambda c: c[3])


def test_table_order_decides_ties(oracle):
    """a flat picture: all nine candidates of a stage tie on distortion (0), so the winner is the first of the cheapest vectors in the stage's
    own table order; the two orders give different winners on some of the cases"""
    W, H, bd = 64, 64, 8
    pic = np.full((H, W), 100, np.int64)
    planes = mr.Planes(pic, bd, 16)
    flat, org, stride = flat_plane(pic)
    differ, real_ties = 0, 0
    for qp in (0, 12, 22, 30):
        sl = mr.sqrt_lambda(oracle, qp, bd)
        for mx in range(-3, 4):
            for my in range(-3, 4):
                r = mr.refine_node(oracle, planes, flat, org, stride, 0, 0, 64, mx, my, sl)
                for stage, table, step, bx, by in (("half", mr.REFINE_H, 2, 4 * mx, 4 * my), ("quarter", mr.REFINE_Q, 1, None, None)):
                    if stage == "quarter":
                        bx, by = min(r["half"], key=lambda c: c[3])[:2]
                    assert all(c[2] == 0 for c in r[stage])
                    costs = [mr.qpel_cost(bx + step * dx, by + step * dy, sl) for dx, dy in table]
                    first = costs.index(min(costs))
                    win = r[stage][first]
                    assert [c[3] for c in r[stage]] == costs
                    if stage == "quarter":
                        assert (r["mvx"], r["mvy"], r["cost_best"]) == (win[0], win[1], win[3])
                    real_ties += costs.count(min(costs)) > 1
                    other = mr.REFINE_Q if stage == "half" else mr.REFINE_H
                    ocosts = [mr.qpel_cost(bx + step * dx, by + step * dy, sl) for dx, dy in other]
                    differ += other[ocosts.index(min(ocosts))] != table[first]
    assert real_ties > 50 and differ > 0


@pytest.mark.parametrize("bd,fx,fy,mv", [(8, 2, 0, (3, -2)), (8, 0, 2, (-1, 4)), (10, 2, 2, (0, 0)), (12, 2, 0, (-5, 1))])
def test_a_half_sample_shift_is_found_exactly(oracle, bd, fx, fy, mv):
    """the current picture IS the reference filtered at a half-sample offset and displaced by an integer vector: from either integer neighbour of
    the true position, every node of every CTU returns the true vector with no distortion left"""
    W, H, qp = 192, 128, 4
    ref = textured(W, H, bd, 21 + bd)
    planes = mr.Planes(ref, bd, 16)
    tx, ty = 4 * mv[0] + fx, 4 * mv[1] + fy                      # the true vector, quarter samples
    a = planes.planes[ty & 3][tx & 3]
    y, x = planes.pad + (ty >> 2), planes.pad + (tx >> 2)
    cur = a[y:y + H, x:x + W].astype(np.int64)
    flat, org, stride = flat_plane(cur)
    cw, ch = frames.ctu_grid(W, H)
    starts = [(mv[0] + sx, mv[1] + sy) for sx in ((0, 1) if fx else (0,)) for sy in ((0, 1) if fy else (0,))]
    checked = 0
    for sx, sy in starts:
        nodes = np.zeros((cw * ch, 85), [("mvx", np.int16), ("mvy", np.int16)])
        nodes["mvx"], nodes["mvy"] = sx, sy
        got = mr.expected(oracle, flat, org, stride, ref, W, H, bd, qp, nodes, 8, planes=planes)
        assert (got["mvx"] == tx).all() and (got["mvy"] == ty).all() and (got["satd_best"] == 0).all()
        assert (got["satd_int"] > 0).all()
        sl = mr.sqrt_lambda(oracle, qp, bd)
        assert (got["cost_best"] == mr.qpel_cost(tx, ty, sl)).all()
        checked += got.size
    assert checked == len(starts) * cw * ch * 85


def test_markers_and_node_order(oracle):
    """nodes crossing the picture edge and vectors beyond max_range carry the marker; node k of a CTU is level / raster as fhevc_motion_node"""
    assert [mr.node_geometry(k) for k in (0, 1, 4, 5, 20, 21, 84)] == [(0, 0, 0), (1, 0, 0), (1, 1, 1), (2, 0, 0), (2, 3, 3), (3, 0, 0), (3, 7, 7)]
    W, H, bd = 96, 64, 8           # two CTUs; the second is 32 samples wide
    ref, cur = textured(W, H, bd, 1), textured(W, H, bd, 2)
    flat, org, stride = flat_plane(cur)
    nodes = np.zeros((2, 85), [("mvx", np.int16), ("mvy", np.int16)])
    nodes["mvx"][0, 21] = 5
    nodes["mvy"][0, 22] = -5
    nodes["mvx"][0, 23] = 4
    got = mr.expected(oracle, flat, org, stride, ref, W, H, bd, 30, nodes, 4)
    marked = got["cost_best"] == mr.MARKER
    assert marked[0].sum() == 2 and marked[0, 21] and marked[0, 22] and not marked[0, 23]
    assert list(marked[1, :5]) == [True, False, True, False, True]
    assert list(marked[1, 5:9]) == [False, False, True, True] and list(marked[1, 21:29]) == [False] * 4 + [True] * 4
    assert marked[1].sum() == 1 + 2 + 8 + 32
    for k in ("satd_int", "satd_best"):
        assert (got[k][marked] == mr.MARKER).all() and (got[k][~marked] != mr.MARKER).all()
    assert (got["mvx"][marked] == 0).all() and (got["mvy"][marked] == 0).all()
