"""The restatement tests/intra_rd_nxn_ref.py of the intra RD stage with the NxN candidate of the 8x8 nodes, held without a GPU: against intra_rd_qt_ref where
there is no candidate or where it cannot win, pictures whose records are known in advance, the choice on hand-set numbers, validity, geometry, bands, and
what the draw of 35 pictures must show at every bit depth."""
import numpy as np
import pytest

import intra_rd_nxn_ref as nx
import intra_rd_qt_ref as iq
import intra_rd_ref as ir
import motion_rd_ref as rd

W, H, N = ir.DRAW_W, ir.DRAW_H, ir.DRAW_N


def invalid_pus(first4):
    """[n, 256] records -> [n, 64]: how many of an 8x8 node's four PUs are invalid by their own bytes"""
    bad = (first4["satd"] == nx.MARK) | ((first4["mode"] & 0xFF) > 34)
    return np.stack([bad[:, nx.units(k)].sum(axis=-1) for k in range(64)], axis=1)


@pytest.mark.parametrize("index", range(0, 35, 6))
def test_without_first4_every_byte_is_the_three_depth_stage(index):
    d = iq.draw(index)
    p, x = nx.plain(d["pic"], d["bd"], d["qp"], d["first"], None)
    assert x is None and p.tobytes() == d["plain"].tobytes()
    for mask in (0, 3):
        a, _ = nx.expected(d["pic"], d["bd"], d["qp"], d["first"], None, d["fold"], d["merge"], mask)
        assert a.tobytes() == iq.expected(d["pic"], d["bd"], d["qp"], d["first"], 3, d["fold"], d["merge"], mask).tobytes()


@pytest.mark.parametrize("index", range(0, 35, 6))
def test_the_nodes_own_mode_four_times_never_wins(index):
    d = iq.draw(index)
    lam = rd.lam_q8(d["qp"])
    first4 = nx.own_first4(d["first"])
    det = {}
    x = nx.candidates(d["pic"], d["bd"], d["qp"], first4, details=det)
    two = d["plain"][:, nx.NODE0:]
    valid = two["part"] != 255
    assert ((x["cost_rd"] != nx.MARK) == valid).all() and valid.sum() > 200
    # J_nxn - (J1 + lam bits(m)) = lam (3 bits(m) - 1): the same four residuals, no split flag, four times the mode's bits
    where3 = {w: m for m, w in enumerate(d["details"][3]["where"])}
    J1 = d["details"][3]["J1"]
    for m, (i, k) in enumerate(det["where"]):
        b = ir.mode_bits(int(d["first"][i, nx.NODE0 + k]["mode"]) & 0xFF)
        j = 256 * int(det["D"][m].sum()) + lam * (int(det["r"][m].sum()) + 4 * b)
        assert j - (int(J1[where3[(i, nx.NODE0 + k)], 0]) + lam * b) == lam * (3 * b - 1)
    # ... so it never wins, and every byte is the stage's without first4
    p, _ = nx.plain(d["pic"], d["bd"], d["qp"], d["first"], first4)
    assert p.tobytes() == d["plain"].tobytes()
    split = valid & (two["tu_split"] == 1)
    assert split.sum() > 20
    bm = np.vectorize(ir.mode_bits)(two["pad"][..., 0])
    assert (x["dist"][split] == two["dist"][split]).all() and (x["bits"][split] == two["bits"][split] - 1 + 3 * bm[split]).all()


@pytest.mark.parametrize("bd,qp", [(8, 22), (10, 37), (12, 51)])
def test_a_constant_picture_with_planar_costs_twelve_lambda_against_four(bd, qp):
    lam = rd.lam_q8(qp)
    pic = iq.constant_picture(64, 64, bd, 1 << (bd - 1))   # the value a line without neighbours takes: the CTU's first row and column are exact too
    p, x = nx.plain(pic, bd, qp, ir.forced(0, (1, 85)), ir.forced(0, (1, 256)))
    assert (x["dist"] == 0).all() and (x["bits"] == 12).all() and (x["cost_rd"] == (12 * lam) >> 8).all() and (x["cbf"] == 0).all() and (x["flags"] == 7).all()
    assert (x["modes"] == 0).all()
    two = p[:, nx.NODE0:]
    assert (two["part"] == ir.PART_INTRA).all() and (two["cost_rd"] == (4 * lam) >> 8).all() and (two["bits"] == 4).all()


@pytest.mark.parametrize("bd,qp", [(8, 27), (10, 32), (12, 22)])
def test_quadrant_stripes_are_exact_for_nxn_alone(bd, qp):
    lam = rd.lam_q8(qp)
    pic = nx.quadrant_stripes(64, 64, bd, 8, 8)
    k = 1 * 8 + 1                                  # the 8x8 node at (8, 8)
    first4 = ir.forced(0, (1, 256))
    first4["mode"][0, nx.units(k)] = nx.STRIPE_MODES
    costs = []
    for m in range(35):
        p, x = nx.plain(pic, bd, qp, ir.forced(m, (1, 85)), first4)
        assert x[0, k]["dist"] == 0 and x[0, k]["bits"] == 4 + 6 + 3 + 6 + 3 and x[0, k]["cost_rd"] == (22 * lam) >> 8 and x[0, k]["cbf"] == 0
        two = iq.plain(pic, bd, qp, ir.forced(m, (1, 85)), 3)[0, nx.NODE0 + k]
        assert two["dist"] > 0 and two["cost_rd"] > x[0, k]["cost_rd"]     # no single mode fits all four quadrants
        costs.append(int(two["cost_rd"]))
        r = p[0, nx.NODE0 + k]
        assert (r["part"], r["dist"], r["cost_rd"], r["bits"], r["flags"], r["tu_split"], r["merged"], tuple(r["pad"])) == \
            (nx.PART_NXN, 0, (22 * lam) >> 8, 22, 7, 1, 0, (0, 0))
    assert min(costs) > (22 * lam) >> 8


def test_the_choice_is_strict_and_an_invalid_2nx2n_loses():
    two = np.zeros(5, nx.PDT)
    two[:] = (500, 1000, 40, 0, 0, ir.PART_INTRA, 0, (26, 0))
    two[3] = ir.MARKER
    x = np.zeros(5, nx.XDT)
    x[:] = (300, 0, 50, 4, 5, (1, 2, 3, 4))
    x["cost_rd"] = [999, 1000, 1001, nx.SAT, nx.MARK]
    x[4] = nx.NXN_MARKER
    outcome = np.zeros(5, np.int64)
    out = nx.choose(two, x, outcome)
    assert outcome.tolist() == [nx.LESS, nx.EQUAL, nx.MORE, nx.ALONE, nx.INVALID]
    assert out["part"].tolist() == [nx.PART_NXN, ir.PART_INTRA, ir.PART_INTRA, nx.PART_NXN, ir.PART_INTRA]
    assert out[1].tobytes() == two[1].tobytes() and out[2].tobytes() == two[2].tobytes() and out[4].tobytes() == two[4].tobytes()
    for i in (0, 3):
        r = out[i]
        assert (r["dist"], r["cost_rd"], r["bits"], r["flags"], r["tu_split"], r["merged"], tuple(r["pad"])) == (300, x["cost_rd"][i], 50, 4, 1, 0, (0, 0))
    # the gate and the fold act on the chosen record: an NxN record one below the fold record is written, an equal one is not
    fold = np.zeros(2, nx.PDT)
    fold[:] = (1, 1000, 1, 0, 0, 2, 0, (0, 0))
    got = ir.gate_fold(np.array([out[0], out[0]]), np.array([fold[0], fold[1]]))
    assert got[0]["part"] == nx.PART_NXN
    fold["cost_rd"] = 999
    assert ir.gate_fold(out[:1], fold[:1])[0]["part"] == 2


def test_one_invalid_pu_gives_the_marker():
    bd, qp = 8, 27
    pic = ir.draw_picture(bd, 3)[:64, :64]
    first = ir.forced(1, (1, 85))
    base = ir.forced(np.arange(256) % 35, (1, 256))
    _, x0 = nx.plain(pic, bd, qp, first, base)
    assert (x0["cost_rd"] != nx.MARK).all()
    a = base.copy()
    a["satd"][0, nx.units(9)[2]] = nx.MARK          # by the marker
    a["mode"][0, nx.units(20)[3]] = 35 | 0x100      # by the mode byte (the high bytes do not count, the low one does)
    a["mode"][0, nx.units(30)[0]] |= 0xABCD00       # high bytes alone change nothing
    p, x = nx.plain(pic, bd, qp, first, a)
    for k in range(64):
        if k in (9, 20):
            assert x[0, k].tobytes() == nx.NXN_MARKER.tobytes() and p[0, nx.NODE0 + k]["part"] == ir.PART_INTRA
        else:
            assert x[0, k].tobytes() == x0[0, k].tobytes()


def test_ragged_72_by_72_prices_the_column_at_64_and_nothing_outside():
    bd, qp = 10, 27
    pic = ir.draw_picture(bd, 4)[:72, :72]
    first, first4 = ir.forced(26, (4, 85)), ir.forced(10, (4, 256))
    p, x = nx.plain(pic, bd, qp, first, first4)
    for c in range(4):
        for k in range(64):
            inside = (c % 2) * 64 + (k % 8) * 8 + 8 <= 72 and (c // 2) * 64 + (k // 8) * 8 + 8 <= 72
            assert (x[c, k]["cost_rd"] != nx.MARK) == inside and (p[c, nx.NODE0 + k]["part"] != 255) == inside
    assert (x[1, ::8]["cost_rd"] != nx.MARK).sum() == 8 and (x[3, 0]["cost_rd"] != nx.MARK)


def test_bands_are_exact_slices():
    d = nx.draw(1)
    for rows in ((0, 1), (1, 3), (2, 3)):
        sl = slice(rows[0] * 3, rows[1] * 3)
        a, x = nx.expected(d["pic"], d["bd"], d["qp"], d["first"][sl], d["first4"][sl], d["fold"][sl], d["merge"][sl], 3, rows)
        full, fx = nx.expected(d["pic"], d["bd"], d["qp"], d["first"], d["first4"], d["fold"], d["merge"], 3)
        assert a.tobytes() == full[sl].tobytes() and x.tobytes() == fx[sl].tobytes()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_draw_shows_every_outcome_at_every_bit_depth(bd):
    counts = np.zeros(5, np.int64)
    one_pu = 0
    for index in range(35):
        if ir.DRAW[index][0] != bd:
            continue
        d = nx.draw(index)
        counts += np.bincount(d["outcome"].ravel(), minlength=5)
        inside = np.zeros((N, 64), bool)
        for c in range(N):
            for k in range(64):
                inside[c, k] = (c % 3) * 64 + (k % 8) * 8 + 8 <= W and (c // 3) * 64 + (k // 8) * 8 + 8 <= H
        one_pu += int((inside & (invalid_pus(d["first4"]) == 1)).sum())
        assert ((d["outcome"] == nx.INVALID) == (~inside | (invalid_pus(d["first4"]) > 0))).all()
    print(bd, "less / equal / more / alone / invalid:", counts.tolist(), "invalid by exactly one PU:", one_pu)
    assert counts[nx.LESS] >= 8 and counts[nx.EQUAL] >= 8 and counts[nx.MORE] >= 8 and counts[nx.ALONE] >= 8 and one_pu >= 8
