"""Pins tests/first_pass_4x4_ref.py -- the expected values tests/test_gpu_first_pass_4x4.py compares the library with -- without a GPU, so that a
mistake in the helper cannot hide on the GPU box.  The helper loops the oracle's fho_first_pass_node(n = 4); here a handful of PUs and modes that
need no predictor code of their own are restated in numpy (a 4x4 Hadamard written with matrices), and the z-order facts of an NxN CU are read off
fho_fill_ref."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import first_pass_4x4_ref as ref4  # noqa: E402
from fasthevc_amd import frames  # noqa: E402
from oracle import oracle_py as op  # noqa: E402

H4 = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], np.int64)


def _satd4(org, pred, bd):
    """xCalcHADs4x4 as xGetHADs calls it: (sum|H d H^T| + 1) >> 1, then >> (bit_depth - 8)"""
    d = org.astype(np.int64) - pred.astype(np.int64)
    return ((int(np.abs(H4 @ d @ H4.T).sum()) + 1) >> 1) >> (bd - 8)


def _picture(W, H, bd, seed):
    rng = np.random.default_rng(seed)
    y = frames.texture16_luma(W, H, seed=seed).astype(np.int16)
    return (y << (bd - 8)) | rng.integers(0, 1 << (bd - 8), size=y.shape).astype(np.int16)


def _cost(satd, mode, sl):
    return float(satd) + float(ref4.MODE_BITS[mode]) * sl


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_helper_against_numpy_on_predictions_that_need_no_predictor(oracle, bd):
    W, H, qp = 104, 72, 30
    pic = _picture(W, H, bd, 3 + bd)
    v = (1 << bd) - 7
    # PU (ux 5, uy 3) of CTU 0 and PU (ux 2, uy 9) of CTU 1: the row above (with the corner) and the column left are one value v, so DC, mode 10
    # and mode 26 all predict v (their edge filters add (v - v) >> 1 and (v + 3v + 2) >> 2)
    spots = [(0, 5, 3), (1, 2, 9)]
    for c, ux, uy in spots:
        x0, y0 = 64 * c + 4 * ux, 4 * uy
        pic[y0 - 1, x0 - 1:x0 + 4] = v
        pic[y0 - 1:y0 + 4, x0 - 1] = v
    flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
    sl = ref4.sqrt_lambda(oracle, qp, bd)
    exp = ref4.expected(oracle, flat, org, stride, W, H, bd, qp)
    # the very first PU of the picture has no neighbour at all: every reference sample is 1 << (bd - 1), DC predicts that value
    s = _satd4(pic[0:4, 0:4], np.full((4, 4), 1 << (bd - 1)), bd)
    e = exp["all"][0, 0, 1]
    assert (e["satd"], e["mode"]) == (s, 1) and e["cost"] == _cost(s, 1, sl)
    # ... and so do planar, 10 and 26 there (flat references)
    for m in (0, 10, 26):
        assert exp["all"][0, 0, m]["satd"] == s and exp["all"][0, 0, m]["cost"] == _cost(s, m, sl)
    for c, ux, uy in spots:
        x0, y0 = 64 * c + 4 * ux, 4 * uy
        s = _satd4(pic[y0:y0 + 4, x0:x0 + 4], np.full((4, 4), v), bd)
        for m in (1, 10, 26):
            e = exp["all"][c, 16 * uy + ux, m]
            assert (e["satd"], e["mode"]) == (s, m) and e["cost"] == _cost(s, m, sl), (c, ux, uy, m)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_helper_best_and_lists_are_consistent(oracle, bd):
    """best = the oracle's own strict-'<' winner = head of the list; the list is the stable order of the helper's costs, restated here as HM's insertion
    (xUpdateCandList: a mode goes behind every entry of smaller or equal cost); ordinary content exercises the tie rule"""
    W, H, qp = 104, 72, 27
    pic = _picture(W, H, bd, 11)
    pic[:16, :24] = 1 << (bd - 1)   # a flat corner: every mode costs satd 0 there
    flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
    exp = ref4.expected(oracle, flat, org, stride, W, H, bd, qp)
    ties, winners, valid = 0, set(), 0
    for c in range(4):
        for pu in range(256):
            if exp["best"][c, pu]["mode"] == 255:
                assert (exp["modes"][c, pu] == 255).all() and (exp["all"][c, pu]["mode"] == 255).all()
                continue
            valid += 1
            cost = exp["all"][c, pu]["cost"]
            lst = []
            for m in range(35):
                pos = len(lst)
                while pos > 0 and cost[m] < cost[lst[pos - 1]]:
                    pos -= 1
                lst.insert(pos, m)
            assert lst[:8] == exp["modes"][c, pu].tolist(), (c, pu)
            b = exp["best"][c, pu]
            assert b["mode"] == lst[0] and b["cost"] == cost[lst[0]] and b["satd"] == exp["all"][c, pu]["satd"][lst[0]]
            ties += len(set(cost[lst[:9]].tolist())) < 9
            winners.add(int(b["mode"]))
    assert valid == (104 // 8) * (72 // 8) * 4
    assert ties >= 50 and len(winners) >= 20, (ties, len(winners))
    assert exp["modes"][0, 0].tolist() == [0, 1, 26, 2, 3, 4, 5, 6]   # the flat corner: mode bits decide, then the mode index


def test_validity_follows_the_8x8_cu(oracle):
    """200 x 100: the height cuts the 8x8 row at y = 96, so its PUs (uy 8, 9 of CTU row 1) are invalid although they lie inside the picture"""
    W, H, bd = 200, 100, 8
    pic = _picture(W, H, bd, 5)
    flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
    exp = ref4.expected(oracle, flat, org, stride, W, H, bd, 32)
    mode = exp["best"]["mode"].reshape(2, 4, 16, 16)   # [cy, cx, uy, ux]
    assert (mode[0] != 255)[:3].all() and (mode[1, :3, :8] != 255).all() and (mode[1, :, 8:] == 255).all()
    assert (mode[:, 3, :, :2] != 255)[0].all() and (mode[:, 3, :, 2:] == 255).all()   # 200 = 3 * 64 + 8: one 8x8 column in the last CTU


@pytest.mark.parametrize("bd", [8, 10])
def test_z_order_inside_one_nxn_cu(oracle, bd):
    """fho_fill_ref at n = 4 inside the 8x8 CU at (40, 24): PU 1 has no below-left (PU 2 comes later), PU 2's above-right is PU 1's bottom row,
    PU 3's above-right lies in the CU to the right, which comes later in z-order, so it is the replicated last sample"""
    W, H = 104, 72
    pic = _picture(W, H, bd, 9)
    flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
    x8, y8 = 40, 24

    def line(x0, y0):
        r = np.zeros(17, np.int16)
        oracle.fho_fill_ref(op.ptr(flat, org), stride, W, H, x0, y0, 4, bd, r)
        return r
    r0, r1, r2, r3 = line(x8, y8), line(x8 + 4, y8), line(x8, y8 + 4), line(x8 + 4, y8 + 4)
    # layout: [0..7] left column bottom to top, [8] corner, [9..16] the row above
    assert r0[9:17].tolist() == pic[y8 - 1, x8:x8 + 8].tolist() and r0[:8].tolist() == pic[y8:y8 + 8, x8 - 1][::-1].tolist()
    assert r1[4:8].tolist() == pic[y8:y8 + 4, x8 + 3][::-1].tolist() and (r1[:4] == r1[4]).all()          # PU 1: below-left replicated
    assert r2[13:17].tolist() == pic[y8 + 3, x8 + 4:x8 + 8].tolist()                                        # PU 2 sees PU 1's samples
    assert r3[9:13].tolist() == pic[y8 + 3, x8 + 4:x8 + 8].tolist() and (r3[13:17] == r3[12]).all()        # PU 3: above-right replicated
    assert len(set(pic[y8 + 3, x8 + 4:x8 + 12].tolist())) > 1 and len(set(pic[y8 + 4:y8 + 8, x8 + 3].tolist())) > 1
