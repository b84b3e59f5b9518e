"""The restatement tests/intra_rd_ref.py of the RD estimate of the intra candidate, held to closed forms without a GPU: pictures whose records are known in
advance, the intra choice rule, every outcome of the calm gate and of the fold built by hand, and what the draw of 35 pictures must show at every level.
The prediction and the transform arithmetic it composes are pinned elsewhere (the oracle's intra functions by the first-pass tests, motion_rd_ref by
tests/test_motion_rd_ref.py); the composition rests on the statements below."""
import numpy as np
import pytest

import intra_rd_ref as ir
import motion_rd_ref as rd

W, H, N = ir.DRAW_W, ir.DRAW_H, ir.DRAW_N
NTU = np.where(ir.LEVEL_OF == 0, 4, 1)[None].repeat(N, 0)


def inside():
    """[N, 85]: the node lies wholly inside the 168 x 152 picture"""
    m = np.zeros((N, 85), bool)
    for c in range(N):
        for k in range(85):
            lvl, bx, by = ir.mr.node_geometry(k)
            s = 64 >> lvl
            m[c, k] = (c % 3) * 64 + (bx + 1) * s <= W and (c // 3) * 64 + (by + 1) * s <= H
    return m


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, qp", [(8, 4), (8, 27), (10, 37), (12, 51)])
def test_a_constant_picture_with_planar(bd, qp):
    """every line is the constant (an unavailable line is 1 << (bd - 1) by definition), planar reproduces it: nothing to code at either depth, and the split
    costs three more flags' worth: J1 - J0 = 3 lam_q8"""
    lam = rd.lam_q8(qp)
    pic = np.full((H, W), 1 << (bd - 1), np.int64)
    got = ir.plain(pic, bd, qp, ir.forced(0))
    v = got["part"] == ir.PART_INTRA
    assert np.array_equal(v, inside()) and v.sum() > 400
    assert (got["dist"][v] == 0).all() and (got["flags"][v] == (ir.ZERO_PLAIN | ir.ZERO_HALF)).all() and (got["tu_split"][v] == 0).all()
    assert (got["bits"][v] == 2 + 2 * NTU[v]).all() and (got["cost_rd"][v] == (lam * (2 + 2 * NTU[v])) >> 8).all()
    assert (got["pad"][v] == (0, 0)).all() and (got["merged"][v] == 0).all()
    assert all(got[~v][f].tolist() == [ir.MARKER[f].tolist()] * int((~v).sum()) for f in ("dist", "cost_rd", "bits", "flags", "tu_split", "part", "merged"))
    detail = {}
    flat = np.full((1, 32, 32), 1 << (bd - 1), np.int64)
    ir.node_records(flat, flat, flat, bd, qp, [2], detail)
    assert (detail["J1"] - detail["J0"] == 3 * lam).all() and not detail["take"].any()


@pytest.mark.parametrize("mode", [26, 10])
def test_stripes_with_the_pure_direction(mode):
    """vertical stripes with mode 26, horizontal stripes with mode 10: where the row above (the column left) is available the prediction is the picture at
    both depths -- the edge filter of N <= 16 adds (side - corner) >> 1 = 0 along a stripe"""
    bd, qp = 8, 22
    yy, xx = np.mgrid[0:H, 0:W]
    pic = ((xx if mode == 26 else yy) * 37 % 251).astype(np.int64)
    detail_of = {}
    got = ir.plain(pic, bd, qp, ir.forced(mode))
    for c in range(N):
        cx, cy = c % 3, c // 3
        for k in range(85):
            lvl, bx, by = ir.mr.node_geometry(k)
            s = 64 >> lvl
            x0, y0 = cx * 64 + bx * s, cy * 64 + by * s
            if x0 + s > W or y0 + s > H:
                assert got[c, k]["part"] == 255
                continue
            available = (y0 > 0) if mode == 26 else (x0 > 0)
            if available:
                assert got[c, k]["dist"] == 0 and got[c, k]["flags"] & 3 == 3 and got[c, k]["tu_split"] == 0 and got[c, k]["bits"] == ir.mode_bits(mode) + 2 * (4 if lvl == 0 else 1), (c, k)
                assert got[c, k]["pad"][0] == mode
                detail_of[lvl] = detail_of.get(lvl, 0) + 1
    assert all(detail_of.get(l, 0) >= 2 for l in range(4))
    P = ir.Picture(pic, bd)
    for n in (32, 16, 8):   # both depths, TU by TU
        assert np.array_equal(P.predict(64, 64, n, mode), pic[64:64 + n, 64:64 + n]) and np.array_equal(P.predict(64 + n, 64 + n, n, mode), pic[64 + n:64 + 2 * n, 64 + n:64 + 2 * n])


def test_invalid_records_give_the_marker():
    bd, qp = 8, 27
    pic = ir.draw_picture(bd, 0)
    first = ir.forced(3)
    first["mode"][0, :40] = 35               # CTUs 0, 1, 3 and 4 lie wholly inside the picture
    first["mode"][1, :40] = 255
    first["satd"][3, :40] = ir.MARK
    first["mode"][0, 40:60] = 0xFFFFFF00 + 36
    first["mode"][4, :40] = 0x1200 + 34      # only the low byte counts: valid
    got = ir.plain(pic, bd, qp, first)
    for c, end in ((0, 60), (1, 40), (3, 40)):
        assert (got[c, :end]["part"] == 255).all() and (got[c, :end]["cost_rd"] == ir.MARK).all() and (got[c, :end]["bits"] == 0xFFFF).all()
        assert got[c, :end].tobytes() == np.full(end, ir.MARKER, ir.PDT).tobytes()
        assert (got[c, end:]["part"] == ir.PART_INTRA).all()
    assert (got[4, :40]["part"] == ir.PART_INTRA).all() and (got[4, :40]["pad"][:, 0] == 34).all()
    assert np.array_equal(got[4, :40], ir.plain(pic, bd, qp, ir.forced(34))[4, :40])


# ---- the choice, the gate, the fold ------------------------------------------------------------------------------------------------------------------------

def test_the_choice_rule_is_strict_and_asks_nothing_of_the_children():
    lam = rd.lam_q8(27)
    # J0 = 256 d0 + lam (1 + r0); the children one less, equal, one more
    d0, r0 = 1000, 40
    for delta, taken in ((-1, True), (0, False), (1, False)):
        j0, j1, take = ir.tu_choice(d0, r0, d0 + delta, r0, lam)
        assert j1 - j0 == 256 * delta and bool(take) == taken
    # a TU whose four children code nothing (r1 = 4: four empty TUs) and still cost less DOES split; the inter rule of fhevc_motion_rd keeps it whole
    j0, j1, take = ir.tu_choice(5000, 1, 100, 4, lam)
    assert j1 < j0 and bool(take)
    assert not bool(rd.tu_choice(5000, 1, 100, 4, False, lam)[2]) and bool(rd.tu_choice(5000, 1, 100, 4, True, lam)[2])
    # through node_records: a 16x16 node whose depth-1 prediction is exact and whose depth-0 prediction is far off
    org = np.full((1, 16, 16), 100, np.int64)
    detail = {}
    dist, cost, bits, flags, tus = ir.node_records(org, org + 40, org, 8, 27, [6], detail)
    assert detail["take"].all() and not detail["any1"].any() and dist[0] == 0 and flags[0] & ir.TU_SPLIT and tus[0] == 1 and bits[0] == 6 + 1 + 4
    assert cost[0] == (lam * (6 + 1 + 4)) >> 8
    # an 8x8 node has one depth
    o8 = np.full((1, 8, 8), 100, np.int64)
    dist, cost, bits, flags, tus = ir.node_records(o8, o8 + 40, None, 8, 27, [6])
    assert tus[0] == 0 and not flags[0] & ir.TU_SPLIT and dist[0] > 0


def rec(cost, part=ir.PART_INTRA, flags=0):
    a = np.zeros(1, ir.PDT)
    a[0] = (cost // 2, cost, 17, flags, 0, part, 0, (5 if part == ir.PART_INTRA else 0, 0)) if part != 255 else ir.MARKER
    return a


def merge_rec(cost, flags):
    a = np.zeros(1, ir.RDT)
    a[0] = (7, cost, 9, flags, 0, 1, -1)
    return a


def test_every_outcome_of_gate_and_fold_by_hand():
    intra, marker = rec(1000), rec(0, 255)
    o = np.zeros(1, int)
    # calm: merge strictly cheaper than the fold record, a masked zero bit -> the fold record stays although intra is cheaper
    fold = rec(2000, 2)
    assert ir.gate_fold(intra, fold, merge_rec(1999, 1), 1, o).tobytes() == fold.tobytes() and o[0] == ir.CALM
    assert ir.gate_fold(intra, fold, merge_rec(1999, 2), 3, o).tobytes() == fold.tobytes() and o[0] == ir.CALM
    # not calm because merge is not strictly cheaper
    assert ir.gate_fold(intra, fold, merge_rec(2000, 3), 3, o).tobytes() == intra.tobytes() and o[0] == ir.INTRA
    assert ir.gate_fold(intra, fold, merge_rec(ir.MARK, 3), 3, o).tobytes() == intra.tobytes()
    # not calm because of the mask (the flag set is not the flag asked for; mask 0 asks for none; bit 2 is no zero bit)
    assert ir.gate_fold(intra, fold, merge_rec(5, 2), 1, o).tobytes() == intra.tobytes() and o[0] == ir.INTRA
    assert ir.gate_fold(intra, fold, merge_rec(5, 3), 0, o).tobytes() == intra.tobytes()
    assert ir.gate_fold(intra, fold, merge_rec(5, 4), 3, o).tobytes() == intra.tobytes()
    # intra cheaper, equal, dearer
    assert ir.gate_fold(intra, rec(1001, 0), None, 0, o).tobytes() == intra.tobytes() and o[0] == ir.INTRA
    for c in (1000, 999):
        f = rec(c, 1)
        assert ir.gate_fold(intra, f, None, 0, o).tobytes() == f.tobytes() and o[0] == ir.KEPT
    # an invalid intra record never replaces anything, a marker fold loses to any valid record
    assert ir.gate_fold(marker, fold, None, 0, o).tobytes() == fold.tobytes() and o[0] == ir.KEPT
    assert ir.gate_fold(intra, marker, None, 0, o).tobytes() == intra.tobytes() and o[0] == ir.INTRA
    assert ir.gate_fold(marker, marker, None, 0).tobytes() == marker.tobytes()
    sat = rec(ir.SAT)
    assert ir.gate_fold(sat, marker, None, 0).tobytes() == sat.tobytes()
    # a marker fold with a calm merge: the marker stays
    assert ir.gate_fold(intra, marker, merge_rec(4000, 1), 1, o).tobytes() == marker.tobytes() and o[0] == ir.CALM
    # no fold: the plain record, or the marker where the node is calm (any merge record that is no marker is cheaper than an absent fold)
    assert ir.gate_fold(intra, None, None, 0, o).tobytes() == intra.tobytes() and o[0] == ir.NO_FOLD
    assert ir.gate_fold(intra, None, merge_rec(4000, 1), 2, o).tobytes() == intra.tobytes() and o[0] == ir.NO_FOLD
    assert ir.gate_fold(intra, None, merge_rec(4000, 1), 1, o).tobytes() == marker.tobytes() and o[0] == ir.CALM
    assert ir.gate_fold(intra, None, merge_rec(ir.MARK, 1), 1, o).tobytes() == intra.tobytes()
    assert ir.gate_fold(marker, None, None, 0).tobytes() == marker.tobytes()


def test_the_fold_into_inter_records_equals_the_plain_form_where_the_fold_is_a_marker():
    bd, qp = 8, 27
    pic = np.full((H, W), 1 << (bd - 1), np.int64)
    p = ir.plain(pic, bd, qp, ir.forced(0))
    fold, _ = ir.draw_inter(p, 3)
    got = ir.expected(pic, bd, qp, ir.forced(0), fold)
    gone = fold["part"] == 255
    assert gone.sum() > 50 and got[gone].tobytes() == p[gone].tobytes()
    assert got[~gone & (fold["cost_rd"] <= p["cost_rd"])].tobytes() == fold[~gone & (fold["cost_rd"] <= p["cost_rd"])].tobytes()


# ---- what the draw shows --------------------------------------------------------------------------------------------------------------------------------------

def test_the_draw_shows_every_case_at_every_level():
    need = 8
    tot = {k: np.zeros(4, int) for k in ir.Stats.KEYS}
    modes = [set() for _ in range(4)]
    filtered = {}
    outcomes = {k: np.zeros(4, int) for k in ("calm", "merge_not_cheaper", "mask", "cheaper", "equal", "dearer", "fold_marker", "no_fold", "no_fold_calm", "invalid_kept")}
    combos = set()
    for index, (bd, qp, _, real) in enumerate(ir.DRAW):
        d = ir.draw(index)
        combos.add((bd, qp))
        for k in tot:
            tot[k] += d["stats"].n[k]
        for l in range(4):
            modes[l] |= d["stats"].modes[l]
        for k, v in d["stats"].filtered.items():
            filtered[k] = filtered.get(k, 0) + v
        p, f, m = d["plain"], d["fold"], d["merge"]
        valid = p["part"] != 255
        pc, fc, mc = p["cost_rd"].astype(np.int64), f["cost_rd"].astype(np.int64), m["cost_rd"].astype(np.int64)
        o = np.zeros(p.shape, int)
        ir.gate_fold(p, f, m, 3, o)
        o2 = np.zeros(p.shape, int)
        ir.gate_fold(p, None, m, 1, o2)
        flagged = (m["flags"] & 3) != 0
        sel = {"calm": o == ir.CALM, "merge_not_cheaper": valid & flagged & (mc >= fc) & (o != ir.CALM), "mask": valid & (mc < fc) & ~flagged,
               "cheaper": (o == ir.INTRA) & (f["part"] != 255), "equal": (o == ir.KEPT) & valid & (pc == fc), "dearer": (o == ir.KEPT) & valid & (pc > fc),
               "fold_marker": (o == ir.INTRA) & (f["part"] == 255), "no_fold": valid & (o2 == ir.NO_FOLD), "no_fold_calm": valid & (o2 == ir.CALM),
               "invalid_kept": ~valid & (o == ir.KEPT)}
        for k, s in sel.items():
            for l in range(4):
                outcomes[k][l] += int(s[:, ir.LEVEL_OF == l].sum())
    assert combos == {(bd, qp) for bd in (8, 10, 12) for qp in ir.DRAW_QPS}
    for k in ("taken", "not_taken"):
        assert (tot[k][:3] >= need).all() and tot[k][3] == 0, (k, tot[k])
    for k in ("clipped", "negative", "dc", "planar", "vertical", "horizontal"):
        assert (tot[k] >= need).all(), (k, tot[k])
    for k, v in outcomes.items():
        assert (v >= need).all(), (k, v)
    # every mode at the three lower levels (level 0 has four nodes a picture), and both filter decisions at every TU size
    assert all(modes[l] == set(range(35)) for l in (1, 2, 3)) and len(modes[0]) >= 20
    assert all(filtered.get((n, use), 0) >= need for n in (32, 16, 8) for use in (0, 1)), filtered
