"""The restatement tests/intra_rd_qt_ref.py of the intra RD estimate on HM's full TU tree, held without a GPU: against intra_rd_ref at two depths, the DST
against the reference's own xTrMxN / xITrMxN with useDST (tests/golden/ref_dst.npz), the nested choice on hand-set numbers, pictures whose records are
known in advance, and what the draw of 35 pictures must show at every level."""
import os

import numpy as np
import pytest

import intra_rd_qt_ref as iq
import intra_rd_ref as ir
import motion_rd_ref as rd

W, H, N = ir.DRAW_W, ir.DRAW_H, ir.DRAW_N
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dst.npz")
LEVEL = ir.LEVEL_OF[None].repeat(N, 0)


def geometry(c, k):
    lvl, bx, by = ir.mr.node_geometry(k)
    s = 64 >> lvl
    return lvl, s, (c % 3) * 64 + bx * s, (c // 3) * 64 + by * s


# ---- against the two-depth module, and the DST against the reference ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("index", range(0, 35, 4))
def test_two_depths_are_the_two_depth_module_byte_for_byte(index):
    d = ir.draw(index)
    assert iq.plain(d["pic"], d["bd"], d["qp"], d["first"], 2).tobytes() == d["plain"].tobytes()
    for mask in (0, 3):
        a = iq.expected(d["pic"], d["bd"], d["qp"], d["first"], 2, d["fold"], d["merge"], mask)
        assert a.tobytes() == ir.expected(d["pic"], d["bd"], d["qp"], d["first"], d["fold"], d["merge"], mask).tobytes()


@pytest.mark.parametrize("index", range(0, 35, 4))
def test_the_64x64_nodes_keep_their_bytes_at_three_depths(index):
    d, q = ir.draw(index), iq.draw(index)
    assert q["plain"][:, 0].tobytes() == d["plain"][:, 0].tobytes()
    assert (q["plain"]["part"] == d["plain"]["part"]).all()                       # validity does not depend on the depth count
    v = q["plain"]["part"] == ir.PART_INTRA
    assert (q["plain"]["pad"][v] == d["plain"]["pad"][v]).all()
    # bits 4..7 only with bit 0, and only at levels 1 and 2
    t = q["plain"]["tu_split"][v]
    assert (((t >> 4) == 0) | ((t & 1) == 1))[LEVEL[v] != 0].all() and ((t >> 4) == 0)[(LEVEL[v] == 0) | (LEVEL[v] == 3)].all() and (t[LEVEL[v] == 3] <= 1).all()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_dst_is_the_references(bd):
    g = np.load(GOLDEN)
    assert bd in g["depths"]
    fin, fco = g[f"fwd_in_{bd}"].astype(np.int64), g[f"fwd_coef_{bd}"].astype(np.int64)
    assert len(fin) >= 10 and np.array_equal(iq.dst_forward(fin, bd), fco)
    co, res = g[f"coef_{bd}"].astype(np.int64), g[f"res_{bd}"].astype(np.int64)
    assert len(co) >= 20 and np.array_equal(iq.dst_inverse(co, bd), res)
    # ... and is not the DCT: the goldens tell the two apart
    assert not np.array_equal(rd.forward(fin, bd), fco) and not np.array_equal(rd.inverse(co, bd), res)
    # fastForwardDst's hard-wired form of HM's earlier versions is the same product (c0 = b0 + b3, c1 = b1 + b3, c2 = b0 - b1, c3 = 74 b2)
    b = np.random.default_rng(bd).integers(-(1 << bd), 1 << bd, size=(50, 4)).astype(np.int64)
    c0, c1, c2, c3 = b[:, 0] + b[:, 3], b[:, 1] + b[:, 3], b[:, 0] - b[:, 1], 74 * b[:, 2]
    fast = np.stack([29 * c0 + 55 * c1 + c3, 74 * (b[:, 0] + b[:, 1] - b[:, 3]), 29 * c2 + 55 * c0 - c3, 55 * c2 - 29 * c1 + c3], axis=1)
    assert np.array_equal(b @ iq.DST.T, fast)


# ---- the nested choice on hand-set numbers -------------------------------------------------------------------------------------------------------------------

def choice(D0, r0, D1, r1, D2, r2, lam, third=True):
    return iq.nested_choice(np.array([D0]), np.array([r0]), np.array([D1]), np.array([r1]), np.array([D2]) if D2 is not None else None,
                            np.array([r2]) if r2 is not None else None, lam, third)


def test_the_nested_choice_is_strict_at_both_depths_and_asks_nothing_of_the_children():
    lam = rd.lam_q8(27)
    quarter = [100, 100, 100, 100]
    # depth 1: K1 = 256 D1 + lam (1 + r1) against K2 = 256 sum D2 + lam (1 + sum r2): one less, equal, one more in D
    for delta, taken in ((-1, True), (0, False), (1, False)):
        ch = choice(10 ** 7, 1, [400 + 0, 400, 400, 400], [9, 9, 9, 9], [[100 + delta, 100, 100, 100], quarter, quarter, quarter], [[3, 2, 2, 2]] * 4, lam)
        assert ch["K2"][0, 0] - ch["K1"][0, 0] == 256 * delta and bool(ch["would1"][0, 0]) == taken and not ch["would1"][0, 1:].any()
        assert bool(ch["take0"][0]) and bool(ch["take1"][0, 0]) == taken
    # depth 0: J1 = sum C + lam against J0, with no depth-1 TU splitting: J1 = 256 * 1600 + lam (1 + 4 * 10)
    for delta, taken in ((-1, False), (0, False), (1, True)):
        ch = choice(1600 + delta, 40, [400] * 4, [9] * 4, [[200] * 4] * 4, [[3] * 4] * 4, lam)
        assert ch["J1"][0] - ch["J0"][0] == -256 * delta and bool(ch["take0"][0]) == taken and not ch["would1"].any()
        assert ch["rate"][0] == (1 + 4 * 10 if taken else 41) and ch["dist"][0] == (1600 if taken else 1600 + delta)
    # a depth-1 TU whose children code nothing (r2 = 1 each) and cost less DOES split -- the inter rule (motion_rd_qt_ref) keeps it whole
    ch = choice(10 ** 7, 1, [5000, 0, 0, 0], [1, 1, 1, 1], [[10, 10, 10, 10], [0] * 4, [0] * 4, [0] * 4], [[1] * 4] * 4, lam)
    assert bool(ch["take1"][0, 0]) and bool(ch["take0"][0]) and ch["dist"][0] == 40 and ch["rate"][0] == 1 + (1 + 4) + 3 * (1 + 1)
    import motion_rd_qt_ref as mq
    inter = mq.nested_choice(np.array([10 ** 7]), np.array([1]), np.array([True]), np.array([[5000, 0, 0, 0]]), np.array([[1, 1, 1, 1]]), np.zeros((1, 4), bool),
                             np.array([[[10, 10, 10, 10], [0] * 4, [0] * 4, [0] * 4]]), np.array([[[1] * 4] * 4]), np.zeros((1, 4, 4), bool), lam)
    assert not inter["would1"].any() and not inter["take0"].any()
    # a depth-0 TU kept although a depth-1 TU would have split: bits 4..7 stay clear
    ch = choice(0, 1, [5000, 0, 0, 0], [1, 1, 1, 1], [[10, 10, 10, 10], [0] * 4, [0] * 4, [0] * 4], [[1] * 4] * 4, lam)
    assert bool(ch["would1"][0, 0]) and not bool(ch["take0"][0]) and not ch["take1"].any()
    dist, cost, bits, flags, tus = iq.node_from_choice({k: v[None] if v.ndim == 1 else v[None] for k, v in ch.items()}, np.zeros((1, 1), bool), np.ones((1, 1), bool), [2], lam)
    assert tus[0] == 0 and not flags[0] & ir.TU_SPLIT and dist[0] == 0 and bits[0] == 2 + 2
    # two depths are the special case: no flag in K1, never a split below
    two = choice(1600, 40, [400] * 4, [9] * 4, None, None, lam, third=False)
    assert two["J1"][0] == 256 * 1600 + lam * (1 + 36) and not two["would1"].any()
    j0, j1, take = ir.tu_choice(1600, 40, 1600, 36, lam)
    assert two["J0"][0] == j0 and two["J1"][0] == j1 and bool(two["take0"][0]) == bool(take)


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, qp", [(8, 4), (10, 27), (12, 51)])
def test_a_constant_picture_with_planar(bd, qp):
    """nothing to code at any depth: J1 - J0 = 7 lam per depth-0 TU of a 32x32 / 16x16 node (four coded-block flags and four split flags against one of
    each, less the one flag more), 3 lam for an 8x8 node, whose depth-1 TUs have no split flag"""
    lam = rd.lam_q8(qp)
    pic = iq.constant_picture(W, H, bd, 1 << (bd - 1))
    details = {}
    got = iq.plain(pic, bd, qp, ir.forced(0), 3, details=details)
    v = got["part"] == ir.PART_INTRA
    assert v.sum() > 400 and (got["dist"][v] == 0).all() and (got["tu_split"][v] == 0).all() and (got["flags"][v] == (ir.ZERO_PLAIN | ir.ZERO_HALF)).all()
    assert got.tobytes() == ir.plain(pic, bd, qp, ir.forced(0)).tobytes()
    for lvl, want in ((0, 3), (1, 7), (2, 7), (3, 3)):
        d = details[lvl]
        assert (d["J1"] - d["J0"] == want * lam).all() and not d["take0"].any() and not d["would1"].any()


@pytest.mark.parametrize("mode", [26, 10])
def test_stripes_with_the_pure_direction(mode):
    """vertical stripes with mode 26, horizontal stripes with mode 10: dist 0 at all three depths wherever the line is available"""
    bd, qp = 8, 22
    pic = iq.stripes(W, H, bd, mode == 26)
    got = iq.plain(pic, bd, qp, ir.forced(mode), 3)
    seen = [0, 0, 0, 0]
    for c in range(N):
        for k in range(85):
            lvl, s, x0, y0 = geometry(c, k)
            if x0 + s > W or y0 + s > H:
                assert got[c, k]["part"] == 255
            elif (y0 > 0) if mode == 26 else (x0 > 0):
                assert got[c, k]["dist"] == 0 and got[c, k]["flags"] & 3 == 3 and got[c, k]["tu_split"] == 0 and got[c, k]["bits"] == 6 - 3 * (mode == 26) + 2 * (4 if lvl == 0 else 1), (c, k)
                seen[lvl] += 1
    assert min(seen) >= 2
    P = ir.Picture(pic, bd)
    for n in (32, 16, 8, 4):   # all depths, TU by TU, the 4x4 line included
        for x0, y0 in ((64, 64), (64 + n, 64 + n), (64 + n, 64)):
            assert np.array_equal(P.predict(x0, y0, n, mode), pic[y0:y0 + n, x0:x0 + n])


@pytest.mark.parametrize("qp, amp", [(4, 20), (22, 60), (27, 100)])
@pytest.mark.parametrize("s, k", [(32, 1 + 2), (16, 5 + 5), (8, 21 + 27)])
def test_a_bump_confined_to_one_4x4_block(s, k, qp, amp):
    """a constant picture with planar and one checkerboard in the LAST 4x4 block of the node -- the one block no TU inside the node takes reference samples
    from, so every TU that does not hold it has a zero residual at every depth.  A 4-sample alternation is 4 x 4 coefficients at N = 4 and spreads over all
    N x N at any larger N, so the path down to the block splits and nothing else: 16x16 -- bit 0 and bit 7 (depth-1 TU 3); 8x8 -- bit 0; 32x32 likewise with
    8x8 TUs, bits 0 and 7"""
    bd = 8
    lvl, s_, x0, y0 = geometry(4, k)
    assert s_ == s
    pic = iq.bumped(W, H, bd, x0 + s - 4, y0 + s - 4, amp)
    details = {}
    got = iq.plain(pic, bd, qp, ir.forced(0), 3, details=details)[4, k]
    assert got["tu_split"] == (1 if s == 8 else 1 | (16 << 3)), got
    assert got["flags"] & ir.TU_SPLIT and not got["flags"] & ir.ZERO_PLAIN
    assert got["cost_rd"] < ir.plain(pic, bd, qp, ir.forced(0))[4, k]["cost_rd"]
    if s != 8:
        d, m = details[lvl], details[lvl]["where"].index((4, k))
        assert (d["K1"][m, 0, :3] == 2 * rd.lam_q8(qp)).all() and (d["K2"][m, 0, :3] == 5 * rd.lam_q8(qp)).all()   # the three other depth-1 TUs: nothing to code


def test_the_dst_changes_the_level_3_records_on_a_bump():
    pic = iq.bumped(W, H, 8, 64 + 24, 64 + 8, 37)
    a, b = iq.plain(pic, 8, 22, ir.forced(0), 3), iq.plain(pic, 8, 22, ir.forced(0), 3, dst=False)
    k = [kk for kk in range(21, 85) if geometry(4, kk)[2:] == (64 + 24, 64 + 8)][0]
    assert a[4, k].tobytes() != b[4, k].tobytes()


# ---- what the draw must show ---------------------------------------------------------------------------------------------------------------------------------

def test_the_draw_shows_every_case_at_every_level():
    """over intra_rd_ref's 35 pictures, at each of levels 1 and 2, each case at least 8 times; 'take0 at two depths but not at three' at least once"""
    keys = ("take1", "keep1", "take1_uncoded", "take0", "keep0", "three_only", "two_only", "kept_though_take1", "cheaper", "dearer")
    n = {l: dict.fromkeys(keys, 0) for l in (1, 2)}
    l3 = dict(taken=0, kept=0, dst_differs=0)
    for index in range(35):
        q = iq.draw(index)
        for l in (1, 2):
            d = q["details"].get(l)
            if d is None:
                continue
            t0, w1, two = d["take0"][:, 0], d["would1"][:, 0], d["two"]["take0"][:, 0]
            c = n[l]
            c["take1"] += int(w1.sum()); c["keep1"] += int((~w1).sum())                      # per depth-1 TU, whatever its parent does
            c["take1_uncoded"] += int((w1 & ~d["cbf2"][:, 0].any(axis=-1)).sum())
            c["take0"] += int(t0.sum()); c["keep0"] += int((~t0).sum())
            c["three_only"] += int((t0 & ~two).sum()); c["two_only"] += int((~t0 & two).sum())
            c["kept_though_take1"] += int((~t0 & w1.any(axis=-1)).sum())
            c["cheaper"] += int((d["J"][:, 0] < d["two"]["J"][:, 0]).sum()); c["dearer"] += int((d["J"][:, 0] > d["two"]["J"][:, 0]).sum())
        d = q["details"].get(3)
        if d is not None:
            l3["taken"] += int(d["take0"].sum()); l3["kept"] += int((~d["take0"]).sum())
            dct = iq.plain(q["pic"], q["bd"], q["qp"], q["first"], 3, dst=False)
            v = (q["plain"]["part"] == ir.PART_INTRA) & (LEVEL == 3)
            l3["dst_differs"] += int((q["plain"][v] != dct[v]).sum())               # the record itself differs: stricter than the sums of the four TUs
    print(n, l3)
    for l in (1, 2):
        for key in keys:
            assert n[l][key] >= (1 if key == "two_only" else 8), (l, key, n[l])
    assert min(l3.values()) >= 8, l3
