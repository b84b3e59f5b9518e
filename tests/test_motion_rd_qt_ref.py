"""The restatement of the RD stages with the depth count (tests/motion_rd_qt_ref.py) without a GPU: at two depths it is motion_rd_ref / motion_rd_pu_ref
on their own draws, every byte; at three the 64x64 and 8x8 nodes keep their bytes; HM's nested choice on hand-set numbers; a zero residual; a residual
confined to one N2 block; and what the 168 x 152 draw holds at levels 1 and 2."""
import numpy as np
import pytest

import motion_rd_pu_ref as pu
import motion_rd_qt_ref as qt
import motion_rd_ref as rd
import motion_refine_ref as mr

DEPTHS = (8, 10, 12)
LEVEL_OF = np.array([mr.node_geometry(k)[0] for k in range(85)])


@pytest.fixture(scope="module")
def draw():
    """per bit depth: the pictures of motion_rd_qt_ref's draw, its three draws of merge records, and per (record seed, QP) the records at 2 and at 3 depths
    with the choice's arrays"""
    out = {}
    for bd in DEPTHS:
        ref, cur = qt.draw_pictures(bd)
        planes = mr.Planes(ref, bd, 16)
        recs = {seed: rd.draw_records(rd.MERGE, seed, 8)[0] for seed in qt.DRAW_RECORD_SEEDS}
        per = {}
        for seed, rec in recs.items():
            for qp in rd.DRAW_QPS:
                details = {}
                two = qt.expected(cur, ref, rd.DRAW_W, rd.DRAW_H, bd, qp, rec, rd.MERGE, 8, 2, planes=planes)
                three = qt.expected(cur, ref, rd.DRAW_W, rd.DRAW_H, bd, qp, rec, rd.MERGE, 8, 3, planes=planes, details=details)
                per[(seed, qp)] = (two, three, details)
        out[bd] = dict(ref=ref, cur=cur, planes=planes, recs=recs, per=per)
    return out


def test_two_depths_are_the_existing_restatements_every_byte(draw):
    for bd in DEPTHS:
        d = draw[bd]
        for qp in rd.DRAW_QPS[::3]:
            base = rd.expected(d["cur"], d["ref"], rd.DRAW_W, rd.DRAW_H, bd, qp, d["recs"][5], rd.MERGE, 8, planes=d["planes"])
            assert d["per"][(5, qp)][0].tobytes() == base.tobytes(), (bd, qp)
    # ... and on motion_rd_ref's own pictures and records, both sources, with and without predictor records
    ref, cur = rd.draw_pictures(8)
    d = dict(ref=ref, cur=cur, planes=mr.Planes(ref, 8, 16))
    rec, _ = rd.draw_records(rd.MERGE, 5, 8)
    base = rd.expected(cur, ref, rd.DRAW_W, rd.DRAW_H, 8, 22, rec, rd.MERGE, 8, planes=d["planes"])
    assert qt.expected(cur, ref, rd.DRAW_W, rd.DRAW_H, 8, 22, rec, rd.MERGE, 8, 2, planes=d["planes"]).tobytes() == base.tobytes()
    q, mvp = rd.draw_records(rd.EXPLICIT, 9, 8, with_mvp=True)
    for m in (None, mvp):
        base = rd.expected(d["cur"], d["ref"], rd.DRAW_W, rd.DRAW_H, 8, 27, q, rd.EXPLICIT, 8, mvp=m, planes=d["planes"])
        assert qt.expected(d["cur"], d["ref"], rd.DRAW_W, rd.DRAW_H, 8, 27, q, rd.EXPLICIT, 8, 2, mvp=m, planes=d["planes"]).tobytes() == base.tobytes()
    # the PU form on the PU module's own draw, forced, selected and folded
    inp = pu.draw_inputs(pu.MAIN_SEED, 8)[0]
    acc = None
    for mode in (0, 2, 5, pu.BEST, pu.SECOND):
        base = pu.expected(d["cur"], d["ref"], pu.W, pu.H, 8, 27, mode, inp, 8, planes=d["planes"], fold_into=acc)
        got = qt.expected_pu(d["cur"], d["ref"], pu.W, pu.H, 8, 27, mode, inp, 8, 2, planes=d["planes"], fold_into=acc)
        assert got.tobytes() == base.tobytes(), mode
        acc = base


def test_levels_0_and_3_keep_their_bytes_at_three_depths(draw):
    changed = 0
    for bd in DEPTHS:
        for key in draw[bd]["per"]:
            two, three, _ = draw[bd]["per"][key]
            keep = (LEVEL_OF == 0) | (LEVEL_OF == 3)
            assert two[:, keep].tobytes() == three[:, keep].tobytes(), (bd, key)
            assert np.array_equal(two["cost_rd"] == rd.MARK, three["cost_rd"] == rd.MARK)
            for f in ("flags", "mvx", "mvy"):
                same = two[f] == three[f] if f != "flags" else (two[f] & 3) == (three[f] & 3)
                assert same.all(), f                                   # bits 0 and 1 are depth-0 properties
            changed += int((two["cost_rd"] != three["cost_rd"]).sum())
            assert ((three["tu_split"] & 0xF0) == 0)[:, keep].all() and ((three["tu_split"] & 0x0E) == 0)[:, LEVEL_OF != 0].all()
            assert ((three["tu_split"] & 0xF0) == 0)[(three["tu_split"] & 1) == 0].all()
            assert np.array_equal((three["flags"] & 4) != 0, (three["tu_split"] & 0x0F) != 0)
    assert changed > 100


# ---- the choice on hand-set numbers ----------------------------------------------------------------------------------------------------------------------

LAM = 1000


def choose(D0, r0, D1, r1, D2, r2, cbf0=None, cbf1=None, cbf2=None, lam=LAM, side=0):
    """one node of one depth-0 TU from plain lists; cbf defaults to r > 1 -> (the choice, the record's five numbers)"""
    D0, r0 = np.array([[D0]]), np.array([[r0]])
    D1, r1 = np.array([[D1]]), np.array([[r1]])
    D2, r2 = np.array([[D2]]), np.array([[r2]])
    cbf0 = r0 > 1 if cbf0 is None else np.array([[cbf0]])
    cbf1 = r1 > 1 if cbf1 is None else np.array([[cbf1]])
    cbf2 = r2 > 1 if cbf2 is None else np.array([[cbf2]])
    ch = qt.nested_choice(D0, r0, cbf0, D1, r1, cbf1, D2, r2, cbf2, lam)
    return ch, tuple(int(v[0]) for v in qt.node_from_choice(ch, cbf0, np.zeros_like(cbf0), [side], lam))


def flat(d2, r2):
    return [[d2] * 4] * 4, [[r2] * 4] * 4


def test_depth_1_one_less_equal_one_more():
    """K1 = 256 D1 + lam (1 + r1) = 256 D1 + 5000 at r1 = 4; K2 = 256 * 4 d2 + lam (1 + 16) at r2 = 4: equal at 1024 d2 + 17000 = 256 D1 + 5000.  D1 = 100 + 12000 / 256
    is no integer, so lam is chosen to make the numbers whole: lam = 256"""
    lam = 256
    # K1 = 256 (D1 + 5), K2 = 256 (4 d2 + 17): equal at D1 = 4 d2 + 12
    for d1, want in ((4 * 10 + 13, True), (4 * 10 + 12, False), (4 * 10 + 11, False)):
        D2, r2 = flat(10, 4)
        ch, rec = choose(10 ** 6, 4, [d1] * 4, [4] * 4, D2, r2, lam=lam)
        assert ch["would1"].all() == want and ch["would1"].any() == want, d1
        assert ch["take0"].all()                                          # the depth-0 TU is far dearer
        assert rec[4] == (1 | 0xF0 if want else 1)
        k = 4 * 10 + 17 if want else d1 + 5
        assert rec[1] == (256 * 4 * k + lam) >> 8 and rec[0] == (160 if want else 4 * d1) and rec[2] == 1 + 4 * (17 if want else 5)


def test_depth_0_one_less_equal_one_more():
    lam = 256
    D2, r2 = flat(10 ** 6, 4)                                              # no depth-1 TU splits
    # J1 = 4 * 256 (20 + 5) + 256 = 256 * 101; J0 = 256 (D0 + 5): equal at D0 = 96
    for d0, want in ((97, True), (96, False), (95, False)):
        ch, rec = choose(d0, 4, [20] * 4, [4] * 4, D2, r2, lam=lam)
        assert not ch["would1"].any() and bool(ch["take0"][0, 0]) == want
        assert rec == ((80, 101, 21, 4, 1) if want else (d0, d0 + 5, 5, 0, 0))


def test_children_that_code_nothing_do_not_split_although_cheaper():
    D2, r2 = flat(1, 1)                                                    # K2 = 256 * 4 + 5 lam, far below K1
    ch, rec = choose(10 ** 6, 4, [10 ** 4] * 4, [4] * 4, D2, r2)
    assert (ch["K2"] < ch["K1"]).all() and not ch["would1"].any() and ch["take0"].all() and rec[4] == 1
    # one coded child among the sixteen: that depth-1 TU alone splits
    r2 = [[1] * 4 for _ in range(4)]
    r2[2][3] = 4
    ch, rec = choose(10 ** 6, 4, [10 ** 4] * 4, [4] * 4, D2, r2)
    assert ch["would1"][0, 0].tolist() == [False, False, True, False] and rec[4] == (1 | 1 << 6)


def test_a_depth_0_tu_coded_only_at_depth_2_splits():
    """no level at depth 0 and none at depth 1; one child at depth 2 holds one and pays: coded_i comes from take1 alone, as HM ORs the cbf upwards"""
    D2 = [[0] * 4 for _ in range(4)]
    r2 = [[1] * 4 for _ in range(4)]
    r2[1][0] = 4
    ch, rec = choose(4100, 1, [1000] * 4, [1] * 4, D2, r2, lam=256)
    assert not ch["coded"][0, 0, [0, 2, 3]].any() and ch["coded"][0, 0, 1] and ch["take0"][0, 0]
    assert rec[4] == (1 | 1 << 5) and rec[3] == (rd.ZERO_PLAIN | rd.TU_SPLIT)
    # J1 = three unsplit (256 * 1000 + 2 lam) + one split (0 + lam (1 + 7)) + lam
    assert rec[1] == (3 * (256 * 1000 + 512) + 256 * 8 + 256) >> 8 and rec[0] == 3000 and rec[2] == 1 + 3 * 2 + 8
    # the same numbers with that child uncoded: nothing is coded anywhere, the TU stays whole although J1 < J0
    r2[1][0] = 1
    ch, rec = choose(4100, 1, [1000] * 4, [1] * 4, D2, r2, lam=256)
    assert (ch["J1"] < ch["J0"]).all() and not ch["take0"].any() and rec == (4100, 4100 + 2, 2, rd.ZERO_PLAIN, 0)


def test_a_depth_0_tu_kept_although_a_depth_1_tu_would_have_split():
    D2, r2 = flat(10, 4)
    ch, rec = choose(100, 4, [5000] * 4, [4] * 4, D2, r2, lam=256)
    assert ch["would1"].all() and not ch["take0"].any() and not ch["take1"].any()
    assert rec == (100, 105, 5, 0, 0)                                      # tu_split bits 4..7 are cleared where bit 0 is clear


def test_a_node_can_cost_more_at_three_depths():
    """depth 0 splits, no depth-1 TU does: four flag bits more than at two depths"""
    lam = 256
    D2, r2 = flat(10 ** 6, 4)
    args = ([[1000]], [[4]], [[True]], [[[20] * 4]], [[[4] * 4]], [[[True] * 4]])
    three = qt.nested_choice(*args, np.array([[D2]]), np.array([[r2]]), np.ones((1, 1, 4, 4), bool), lam)
    two = qt.nested_choice(*args, None, None, None, lam, third=False)
    assert three["take0"].all() and two["take0"].all() and not three["take1"].any()
    assert int(three["J"][0, 0] - two["J"][0, 0]) == 4 * lam and int(three["rate"][0, 0] - two["rate"][0, 0]) == 4
    assert int(three["dist"][0, 0]) == int(two["dist"][0, 0]) == 80


def test_both_saturations():
    D2, r2 = flat(10, 4)
    big = 1 << 31
    ch, rec = choose(big, 40000, [big] * 4, [40000] * 4, D2, [[30000] * 4] * 4, lam=1 << 20)
    assert rec[2] == 65535                                                  # bits
    ch, rec = choose(0xFFFFFFFF, 4, [0xFFFFFFFF] * 4, [4] * 4, [[0x3FFFFFFF] * 4] * 4, r2, lam=1 << 30)
    assert rec[1] == rd.SAT                                                 # cost_rd: never the marker's number
    ch, rec = choose(100, 4, [5000] * 4, [4] * 4, D2, r2, lam=256, side=70000)
    assert rec[2] == 65535 and rec[1] == 105 + 70000


# ---- constructed residuals -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", (32, 16))
def test_a_zero_residual_gives_the_two_depth_record(s):
    rng = np.random.default_rng(s)
    org = rng.integers(0, 256, size=(3, s, s))
    for qp in (4, 27, 51):
        assert all(np.array_equal(a, b) for a, b in zip(qt.node_records(org, org, 8, qp, [3, 4, 5], 3), rd.node_records(org, org, 8, qp, [3, 4, 5])))


@pytest.mark.parametrize("s", (32, 16))
def test_a_residual_confined_to_one_N2_block_splits_down_to_it(s):
    for i in range(4):
        for sub in (0, 3):
            org, pred = qt.confined_node(s, i, sub)
            three = qt.node_records(org[None], pred[None], 8, 22, [2], 3)
            two = rd.node_records(org[None], pred[None], 8, 22, [2])
            assert int(three[4][0]) == (1 | 1 << (4 + i)), (s, i, sub, three)
            assert int(three[1][0]) < int(two[1][0]) and int(two[4][0]) == 1


def test_a_real_residual_where_the_cbf_condition_of_depth_1_decides():
    """the constructed 12-bit node: depth-1 TU 1 is coded, its children are not and are cheaper, and it stays whole; without the condition it would split"""
    org, pred = qt.unpaid_node()
    detail = {}
    rec = qt.node_records(org[None], pred[None], qt.UNPAID_BD, qt.UNPAID_QP, [2], 3, detail)
    assert detail["cbf1"][0, 0].tolist() == [False, True, True, False] and (detail["K2"] < detail["K1"])[0, 0, 1] and not detail["would1"][0, 0, 1]
    assert detail["take0"][0, 0] and int(rec[4][0]) == 1 and int(rec[2][0]) == 64
    lam = rd.lam_q8(qt.UNPAID_QP)
    assert int(detail["K1"][0, 0, 1]) == 7 * lam and int(detail["K2"][0, 0, 1]) == 5 * lam       # D = 0 on both sides: r1 = 6 against four children of r = 1


# ---- the draw --------------------------------------------------------------------------------------------------------------------------------------------

def test_the_draw_holds_every_case_at_levels_1_and_2(draw):
    names = ("split1_under_split0", "kept1_under_split0", "kept0_although_K2_below_K1", "coded_only_at_depth_2", "cheaper", "dearer")
    n = {lvl: dict.fromkeys(names, 0) for lvl in (1, 2)}
    for bd in DEPTHS:
        for key in draw[bd]["per"]:
            two, three, details = draw[bd]["per"][key]
            for lvl in (1, 2):
                d = details[lvl]
                t0, w1 = d["take0"][:, 0], d["would1"][:, 0]
                c = n[lvl]
                c["split1_under_split0"] += int((t0[:, None] & w1).sum())
                c["kept1_under_split0"] += int((t0[:, None] & ~w1).sum())
                c["kept0_although_K2_below_K1"] += int((~t0 & (d["K2"][:, 0] < d["K1"][:, 0]).any(axis=-1)).sum())
                c["coded_only_at_depth_2"] += int((t0 & ~d["cbf0"][:, 0] & ~d["cbf1"][:, 0].any(axis=-1)).sum())
                sel = LEVEL_OF == lvl
                a, b = two["cost_rd"][:, sel].astype(np.int64), three["cost_rd"][:, sel].astype(np.int64)
                c["cheaper"] += int((b < a).sum())
                c["dearer"] += int((b > a).sum())
    assert all(v >= 8 for lvl in (1, 2) for v in n[lvl].values()), n
