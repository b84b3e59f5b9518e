"""The restatement tests/intra_rd_search_ref.py held to the definition without a GPU: the identities of the header's section, HM's best / second bookkeeping on
hand-set sequences, the planar append, the positions in pad[1], pictures whose result is known in advance, the ragged picture and bands as slices."""
import numpy as np

import intra_rd_nxn_ref as nx
import intra_rd_qt_ref as iq
import intra_rd_ref as ir
import intra_rd_search_ref as sr
import motion_rd_ref as rd

import pytest

OUTCOMES = ("not0", "second", "planar")
FLOOR = 8


def test_best_and_second_as_hm_keeps_them():
    assert sr.best_second([]) == (None, None)
    assert sr.best_second([5]) == (0, None)
    assert sr.best_second([1, 2, 3, 4]) == (0, 1)            # ascending: the first two
    assert sr.best_second([4, 3, 2, 1]) == (3, 2)            # descending: every new best demotes the old one
    assert sr.best_second([3, 3, 3]) == (0, 1)               # ties: not strictly below the best; the first of them is below no second yet, the next is not below it
    assert sr.best_second([5, 9, 7, 5, 6]) == (0, 3)         # a tie with the best becomes the second (strictly below 7)
    assert sr.best_second([5, 9, 1]) == (2, 0)               # the demoted best replaces a dearer second
    assert sr.best_second([2, 1, 9, 0]) == (3, 1)


def test_the_list_of_a_node_and_the_planar_append():
    e = np.array([10, 200, 26, 0, 1, 2, 3, 4], np.uint8)
    assert sr.candidates_of(e, 3, 1) == [(0, 10), (2, 26), (3, 0)]                 # appended, at the position behind the last byte used; the byte > 34 is skipped
    assert sr.candidates_of(e, 4, 1) == [(0, 10), (2, 26), (3, 0)]                 # not appended: 0 is in the list
    assert sr.candidates_of(np.array([35, 255, 99], np.uint8), 3, 1) == []         # not appended: the list is empty
    assert sr.candidates_of(e, 3, 0) == [(0, 10), (2, 26)]                         # append_planar 0
    assert sr.candidates_of(e, 1, 1) == [(0, 10), (1, 0)]
    assert sr.candidates_of(np.array([7, 7, 7], np.uint8), 3, 0) == [(0, 7), (1, 7), (2, 7)]   # duplicates are priced again


@pytest.mark.parametrize("index", range(len(ir.DRAW)))
def test_identities_on_the_draw(index):
    one = dict(count=(1, 1, 1, 1), count4=1, append_planar=0)
    d = sr.draw(index)
    bd, qp = d["bd"], d["qp"]
    first, first4 = sr.first_of(d["modes"]), sr.first_of(d["modes4"])
    # (i) counts 1, no append: the NxN stage fed the lists' first bytes, with and without the 4x4 input, through gate and fold
    for with4 in (True, False):
        got, gx = sr.expected(d["pic"], bd, qp, d["modes"], d["modes4"] if with4 else None, one, d["fold"], d["merge"], 3)
        exp, ex = nx.expected(d["pic"], bd, qp, first, first4 if with4 else None, d["fold"], d["merge"], 3)
        assert got.tobytes() == exp.tobytes() and (gx is None) == (ex is None) and (gx is None or gx.tobytes() == ex.tobytes())
    # (ii) the record of any node is the three-depth stage's for the winning mode, in all bytes but pad[1]
    two = sr.plain(d["pic"], bd, qp, d["modes"], None, sr.DEFAULT)[0]
    win = np.zeros(two.shape, sr.NDT)
    win["mode"] = np.where(two["part"] == 255, 255, two["pad"][..., 0])
    q = iq.plain(d["pic"], bd, qp, win, 3)
    z = two.copy()
    z["pad"][..., 1] = 0
    assert z.tobytes() == q.tobytes()
    # (iii) F(m).J <= A(m) at every mode, so the result never costs more than step A's cost of the list's first valid entry (it MAY cost more than F of
    # that entry: HM's two steps rank on A, and a mode ranked third on A is never tried on the full tree)
    P = ir.Picture(d["pic"], bd)
    at = sr._per_mode(P, bd, qp, two.shape[0], (0, (P.H + 63) // 64))
    a0 = np.zeros(two.shape, np.int64)
    for m in range(35):
        rec, J, A = at(m)
        assert (J <= A).all(), m
        sel = (first["mode"] == m) & (two["part"] != 255)
        a0[sel] = A[sel]
    ok = (two["part"] != 255) & (first["mode"] <= 34)
    assert (two["cost_rd"][ok].astype(np.int64) <= np.minimum(a0[ok] >> 8, sr.SAT)).all()


def outcome_counts():
    """what the draw shows -> {(outcome, bit depth or None, level or "pu")}: per bit depth and per level 1..3, over the draw as a whole for level 0 and the PUs"""
    counts = {}

    def add(key, n):
        counts[key] = counts.get(key, 0) + int(n)
    for index in range(len(ir.DRAW)):
        d = sr.draw(index)
        st, bd = d["stats"], d["bd"]
        got = {"not0": st["pos"] > 0, "second": st["second_won"], "planar": st["planar_won"]}
        for name, hit in got.items():
            add((name, None, 0), hit[:, sr.LEVEL == 0].sum())
            for lvl in (1, 2, 3):
                add((name, bd, lvl), hit[:, sr.LEVEL == lvl].sum())
        inside = st["pu_mode"] <= 34
        add(("pu_mode_differs_from_its_first_byte", None, "pu"), (st["pu_mode"][inside] != d["modes4"][..., 0][inside]).sum())
        firsts = nx.plain(d["pic"], bd, d["qp"], sr.first_of(d["modes"]), sr.first_of(d["modes4"]))[0]
        add(("nxn_wins_where_it_lost_under_first_bytes", None, "pu"), ((d["plain"][:, 21:]["part"] == nx.PART_NXN) & (firsts[:, 21:]["part"] != nx.PART_NXN)).sum())
    return counts


def test_what_the_draw_shows_reaches_every_floor():
    counts = outcome_counts()
    print(sorted(counts.items(), key=str))
    assert len(counts) == 3 * (1 + 9) + 2
    short = {k: v for k, v in counts.items() if v < FLOOR}
    assert not short, short


def test_pad1_positions_and_the_constant_picture():
    bd, qp = 8, 27
    lam = rd.lam_q8(qp)
    flat = iq.constant_picture(64, 64, bd, 1 << (bd - 1))
    modes = np.tile(np.array([10, 26, 5, 7, 9, 11, 13, 15], np.uint8), (1, 85, 1))
    modes4 = np.tile(np.array([10, 26, 5, 7, 9, 11, 13, 15], np.uint8), (1, 256, 1))
    p, x = sr.plain(flat, bd, qp, modes, modes4)
    # every mode predicts the constant picture exactly: the cheapest flag wins -- the appended planar, at position count[l]
    assert (p[0, 1:]["dist"] == 0).all() and (p[0, 1:]["pad"][:, 0] == 0).all() and (p[0, 1:21]["pad"][:, 1] == 3).all() and (p[0, 21:]["pad"][:, 1] == 8).all()
    assert (p[0, 21:]["cost_rd"] == (4 * lam) >> 8).all() and (p[0, 21:]["part"] == ir.PART_INTRA).all()
    assert (x["dist"] == 0).all() and (x["bits"] == 12).all() and (x["cost_rd"] == (12 * lam) >> 8).all() and (x["modes"] == 0).all()
    # without the append the dearer flags tie: the list's first entry stays (26 costs 3 bits, below 10's 6: position 1)
    p, _ = sr.plain(flat, bd, qp, modes, None, dict(count=(3, 3, 3, 8), count4=8, append_planar=0))
    assert (p[0, 1:]["pad"][:, 0] == 26).all() and (p[0, 1:]["pad"][:, 1] == 1).all()


def test_the_stripe_picture_with_the_right_modes_last():
    bd, qp = 8, 27
    pic = nx.quadrant_stripes(64, 64, bd, 8, 8)
    modes = np.full((1, 85, 8), 1, np.uint8)
    m4 = np.full((1, 256, 8), 1, np.uint8)
    m4[0, nx.units(9), 7] = nx.STRIPE_MODES
    _, x = sr.plain(pic, bd, qp, modes, m4, dict(count=(3, 3, 3, 8), count4=8, append_planar=0))
    assert x[0, 9]["dist"] == 0 and tuple(x[0, 9]["modes"]) == nx.STRIPE_MODES


def test_the_ragged_picture_and_bands_as_slices():
    bd, qp = 10, 30
    rng = np.random.default_rng(5)
    pic = rng.integers(0, 1 << bd, size=(72, 72)).astype(np.int16)
    modes, modes4 = sr.random_lists(rng, 4, 85), sr.random_lists(rng, 4, 256)
    p, x = sr.plain(pic, bd, qp, modes, modes4)
    # nodes outside 72 x 72 carry the marker, whatever their lists hold
    assert (p[1, 1:]["part"] == 255).sum() > 60 and p[0, 0]["part"] != 255 and p[3, 0]["part"] == 255
    for rows in ((0, 1), (1, 2)):
        sl = slice(rows[0] * 2, rows[1] * 2)
        q, y = sr.plain(pic, bd, qp, modes[sl], modes4[sl], rows=rows)
        assert q.tobytes() == p[sl].tobytes() and y.tobytes() == x[sl].tobytes()
