"""The restatement of the RD stage (tests/motion_rd_ref.py) held to the reference's own transforms -- forward (tests/golden/ref_transform.npz, and
ref_inverse_transform.npz for N = 4) and inverse (ref_inverse_transform.npz, written by tests/quality/gen_inverse_transform_golden.py from calls into
xTrMxN and xITrMxN) --, to the reference's own quantiser for the levels (ref_quant.npz), to closed forms, to hand-written choices, and to
motion_skip_ref's two zero bits on a draw that is shown to exercise every branch -- without a GPU.  tests/test_gpu_motion_rd.py compares the kernel with
this restatement, so what is pinned here is what the kernel is held to.  NOT pinned to the reference: xDeQuant (a member function) and xQuant at N = 4
(it needs a live TU); both rest on the restatement of the cited lines, and the bit estimate is the library's own."""
import os

import numpy as np
import pytest

import motion_refine_ref as mr
import motion_rd_ref as rd
import motion_skip_quant_cases as qc
import motion_skip_ref as sk

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES, DEPTHS = (4, 8, 16, 32), (8, 10, 12)


@pytest.fixture(scope="module")
def forward_golden():
    return np.load(os.path.join(HERE, "golden", "ref_transform.npz"))


@pytest.fixture(scope="module")
def inverse_golden():
    return np.load(os.path.join(HERE, "golden", "ref_inverse_transform.npz"))


@pytest.fixture(scope="module")
def draw():
    """per bit depth: the pictures, the merge records, and per QP the expected records with what they exercised"""
    out = {}
    for bd in DEPTHS:
        ref, cur = rd.draw_pictures(bd)
        planes = mr.Planes(ref, bd, 16)
        rec, _ = rd.draw_records(rd.MERGE, 5, 8)
        per_qp = {}
        for qp in rd.DRAW_QPS:
            st = rd.Stats()
            per_qp[qp] = (rd.expected(cur, ref, rd.DRAW_W, rd.DRAW_H, bd, qp, rec, rd.MERGE, 8, planes=planes, stats=st), st)
        out[bd] = dict(ref=ref, cur=cur, planes=planes, rec=rec, per_qp=per_qp)
    return out


# ---- the transforms -----------------------------------------------------------------------------------------------------------------------------------------

def test_the_recorded_tables_are_the_restated_ones(forward_golden, inverse_golden):
    g = inverse_golden
    assert tuple(g["sizes"]) == SIZES and tuple(g["depths"]) == DEPTHS
    assert tuple(int(v) for v in g["inv_quant_scales"]) == rd.INV_QUANT_SCALES == (40, 45, 51, 57, 64, 72)
    assert np.array_equal(rd.matrix(4), g["matrix4"]) and np.array_equal(rd.matrix(4), rd.matrix(32)[::8, :4])
    for n in (8, 16, 32):
        assert np.array_equal(rd.matrix(n), forward_golden[f"matrix{n}"])
    assert all(a.dtype.kind in "iu" for a in g.values())                # integers only
    # the N-point transposes are no sub-blocks of the 32-point transpose: why the kernel keeps one table per size
    assert all(not np.array_equal(rd.matrix(n).T, rd.matrix(32).T[:n, :n]) for n in (4, 8, 16))


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("n", SIZES)
def test_the_forward_transform_equals_the_reference(forward_golden, inverse_golden, n, bd):
    blocks, coefs = (inverse_golden[f"fwd_in_4_{bd}"], inverse_golden[f"fwd_coef_4_{bd}"]) if n == 4 else (forward_golden[f"in_{n}_{bd}"], forward_golden[f"coef_{n}_{bd}"])
    assert len(blocks) >= 13 and np.abs(blocks).max() == (1 << bd) - 1
    got = rd.forward(blocks.astype(np.int64), bd)                        # batched: the module's own form
    assert np.array_equal(got, coefs), (n, bd, np.argwhere(got != coefs)[:5])
    if n >= 8:
        assert all(np.array_equal(sk.forward(b, bd), c) for b, c in zip(blocks, got))     # ... and the skip stage's restatement says the same


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("n", SIZES)
def test_the_inverse_transform_equals_the_reference(inverse_golden, n, bd):
    coef, res = inverse_golden[f"coef_{n}_{bd}"].astype(np.int64), inverse_golden[f"res_{n}_{bd}"].astype(np.int64)
    # the cases the file promises: the full 16-bit range with its extremes, impulses, DC only, the first-stage clip (and at 12 bit the second)
    assert len(coef) >= 15 and coef.min() == -32768 and coef.max() == 32767 and (coef == -32767).any()
    assert sum(1 for c in coef if np.count_nonzero(c) == 1) >= 8 and sum(1 for c in coef if np.count_nonzero(c) == 1 and c[0, 0]) >= 3
    tmp, got = rd.inverse(coef, bd, stages=True)
    assert np.array_equal(got, res), (n, bd, np.argwhere(got != res)[:5])
    m = rd.matrix(n)
    unclipped = (np.swapaxes(coef, -1, -2) @ m + 64) >> 7
    assert (unclipped > 32767).any() and (unclipped < -32768).any() and tmp.max() == 32767 and tmp.min() == -32768
    if bd == 12 and n >= 8:
        assert (np.abs(res) >= 32767).any()                              # the Pel clip of the second stage was reached as well


@pytest.mark.parametrize("bd", DEPTHS)
def test_sixteen_bit_intermediates_at_n_4_and_the_inverse_accumulations(forward_golden, inverse_golden, bd):
    """forward at N = 4 from the recorded matrix's absolute row sums, as test_motion_skip_ref.py does for the larger sizes; inverse: the inputs of either
    stage are 16-bit by their clips, so an accumulation is at most 32768 times a column's absolute sum"""
    m = inverse_golden["matrix4"].astype(np.int64)
    rows = np.abs(m).sum(axis=1)
    s1, s2 = sk.shifts(4, bd)
    first = (int(rows.max()) * ((1 << bd) - 1) + (1 << (s1 - 1))) >> s1
    second = (int(rows.max()) * first + (1 << (s2 - 1))) >> s2
    assert int(rows.max()) == 64 * 4 and first <= 32767 and second <= 32767
    tmp, out = rd.forward(np.full((4, 4), (1 << bd) - 1), bd, stages=True)
    assert int(np.abs(tmp).max()) == first and int(np.abs(out).max()) == second
    tmp, out = rd.forward(np.full((4, 4), -((1 << bd) - 1)), bd, stages=True)
    assert tmp.min() >= -32768 and out.min() >= -32768
    for n in SIZES:
        mat = (inverse_golden["matrix4"] if n == 4 else forward_golden[f"matrix{n}"]).astype(np.int64)
        worst = 32768 * int(np.abs(mat).sum(axis=0).max()) + (1 << 11)
        assert worst <= 32 * 32768 * 90 + (1 << 11) < 2 ** 31, n


# ---- quantiser and dequantiser ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", qc.DEPTHS)
@pytest.mark.parametrize("n", qc.SIZES)
def test_depth_0_levels_are_the_references_at_every_qp(n, bd):
    g = np.load(qc.GOLDEN)
    i, j = qc.SIZES.index(n), qc.DEPTHS.index(bd)
    for qp in qc.ALL_QPS:
        c = np.concatenate([g["thr_special"][i, j, qp], g["thr_random"].astype(np.int32)]).astype(np.int64)
        assert np.array_equal(rd.levels(c, n, bd, qp), g["thr_levels"][i, j, qp].astype(np.int64)), (n, bd, qp)


def test_right_shift_target_input_bit_depth_and_the_level_bound():
    seen = {n: set() for n in SIZES}
    for n in SIZES:
        for bd in range(8, 13):
            for qp in range(52):
                rs = rd.right_shift(n, bd, qp)
                assert rs == rd.log2(n) - 1 - qp // 6                    # no bit depth in it
                assert rd.target_input_bit_depth(n, bd, qp) == 16       # 32 + rightShift - 7 >= 18: the min is maxLog2TrDynamicRange + 1
                scale, qbits, add_plain, _ = sk.quant(n, bd, qp)
                assert (32768 * scale + add_plain) >> qbits <= 13108     # the int16 clip of the level never binds
                if bd == 8 and qp in rd.DRAW_QPS:
                    seen[n].add((rs > 0) - (rs < 0))
    # the draw's QPs bring every TU size to a positive, a zero and a negative rightShift
    assert all(s == {-1, 0, 1} for s in seen.values()), seen
    # the two branches agree where they meet, and the rounding is HM's
    assert rd.dequant(np.array([3, -3]), 8, 8, 4).tolist() == [(3 * 64 + 2) >> 2, (-3 * 64 + 2) >> 2]      # rightShift 2, rem 4
    assert rd.dequant(np.array([3, -3]), 8, 8, 14).tolist() == [3 * 51, -3 * 51]                          # rightShift 0, rem 2
    assert rd.dequant(np.array([3, -3]), 8, 8, 37).tolist() == [(3 * 45) << 4, -((3 * 45) << 4)]          # rightShift -4, rem 1
    assert rd.dequant(np.array([32767, -32768]), 4, 8, 51).tolist() == [32767, -32768]                     # the clip of the result


# ---- closed forms -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", DEPTHS)
def test_a_zero_residual_costs_the_cbf_bits_only(bd):
    rng = np.random.default_rng(bd)
    for s in (64, 32, 16, 8):
        org = rng.integers(0, 1 << bd, size=(3, s, s))
        for qp in (0, 22, 51):
            detail = {}
            dist, cost, bits, flags, tus = rd.node_records(org, org, bd, qp, [2, 2, 2], detail)
            t = 4 if s == 64 else 1
            assert (dist == 0).all() and (detail["r0"] == 1).all() and (detail["r1"] == 4).all() and not detail["take"].any()
            assert (bits == t * 2 + 2).all()                             # per TU the cbf bit and the split flag's, + side_bits
            assert (cost == (rd.lam_q8(qp) * (2 * t + 2)) >> 8).all() and (flags == 3).all() and (tus == 0).all()


@pytest.mark.parametrize("bd", DEPTHS)
def test_a_constant_residual_is_dc_only_and_a_dequantised_basis_rebuilds_exactly(bd):
    for n in SIZES:
        c = rd.forward(np.full((n, n), 5), bd)
        assert c[0, 0] == 5 << (15 - bd) and np.count_nonzero(c) == 1
        # level 3 at DC, at a QP whose rightShift is not positive: c^ = 3 * 64 << k is a multiple of 2^(bd - 3): the inverse is exact in both stages
        qp = 6 * (rd.log2(n) + 2) + 4
        chat = np.zeros((n, n), np.int64)
        chat[0, 0] = int(rd.dequant(np.array([3]), n, bd, qp)[0])
        assert rd.right_shift(n, bd, qp) == -3 and chat[0, 0] == 3 * 64 * 8
        r = rd.inverse(chat, bd)
        value = 3 * 64 * 8 >> (15 - bd)
        assert (r == value).all() and value > 0
        # ... so a residual that IS that block quantises to level 3 and rebuilds with D = 0
        org = np.full((1, n, n), 100 + value)
        pred = np.full((1, n, n), 100)
        p = rd.tu_pass(org, pred, bd, qp)
        assert p["levels"][0, 0, 0] == 3 and np.count_nonzero(p["levels"]) == 1 and p["D"][0] == 0 and p["r"][0] == 1 + 3 + 2


# ---- the choice ---------------------------------------------------------------------------------------------------------------------------------------------

def test_lambda_in_q8():
    assert rd.lam_q8(12) == 146 and rd.lam_q8(22) == 1471 and rd.lam_q8(0) == 9 and rd.lam_q8(51) == int(0.57 * 2 ** 13 * 256 + 0.5)
    assert all(rd.lam_q8(q) < rd.lam_q8(q + 1) for q in range(51))


def test_a_split_taken_with_both_costs_written_out_by_hand():
    """an 8x8 node at 8 bit, QP 22 (lam_q8 1471; N = 4: qbits 22, scale 16384; rightShift -2, inverse scale 64), flat prediction 128, the residual 10 on
    the top-left 4x4 child and 0 elsewhere.
    Depth 1: that child is DC only, c = 10 << 7 = 1280; level = (1280 * 16384 + (85 << 13)) >> 22 = 5; c^ = (5 * 64) << 2 = 1280; first inverse stage
    (64 * 1280 + 64) >> 7 = 640, second (64 * 640 + 2048) >> 12 = 10: rebuilt exactly, D = 0, r = 1 + 3 + 2 * 2 = 8; the other children r = 1, D = 0.
    J1 = 256 * 0 + 1471 * (1 + 11) = 17652.
    Depth 0 (N = 8: qbits 21): the 8x8 transform spreads the quadrant over the odd frequencies; the four lowest coefficients 320, 290, 290, 263 quantise to
    level 2 each ((320 * 16384 + (85 << 12)) >> 21 = 2, (263 * 16384 + (85 << 12)) >> 21 = 2) and the next largest, 102, to 0: r0 = 1 + 4 * (3 + 2) = 21; the
    four levels rebuild a ramp instead of the step, D0 = 290.  J0 = 256 * 290 + 1471 * (1 + 21) = 106602.
    J1 < J0 and a child is coded: the split is taken, cost_rd = (17652 + 1471 * side_bits) >> 8."""
    org = np.full((1, 8, 8), 128)
    org[0, :4, :4] += 10
    pred = np.full((1, 8, 8), 128)
    child = rd.tu_pass(org[:, :4, :4], pred[:, :4, :4], 8, 22)
    assert rd.forward(org[0, :4, :4] - 128, 8)[0, 0] == 1280 and child["levels"][0, 0, 0] == 5 and child["D"][0] == 0 and child["r"][0] == 8
    detail = {}
    dist, cost, bits, flags, tus = rd.node_records(org, pred, 8, 22, [3], detail)
    assert detail["J1"][0, 0] == 17652 == 1471 * 12 and detail["r1"][0, 0] == 11 and detail["D1"][0, 0] == 0
    c0 = rd.forward(org[0] - 128, 8)
    assert c0[:2, :2].tolist() == [[320, 290], [290, 263]] and (320 * 16384 + (85 << 12)) >> 21 == 2 == (263 * 16384 + (85 << 12)) >> 21 and (102 * 16384 + (85 << 12)) >> 21 == 0
    assert np.count_nonzero(detail["levels0"]) == 4 and (detail["levels0"][0, 0, :2, :2] == 2).all()
    assert (int(detail["D0"][0, 0]), int(detail["r0"][0, 0])) == (290, 21) and detail["J0"][0, 0] == 256 * 290 + 1471 * 22 == 106602
    assert detail["take"][0, 0] and tus[0] == 1 and flags[0] == rd.TU_SPLIT and dist[0] == 0 and bits[0] == 12 + 3
    assert cost[0] == (17652 + 1471 * 3) >> 8


def test_equal_costs_do_not_split_and_the_comparison_is_strict():
    """lam_q8(12) = 146 and 146 * 128 = 256 * 73: with 128 more bits and 73 less distortion the children cost exactly the parent's J"""
    lam = rd.lam_q8(12)
    j0, j1, take = rd.tu_choice([1000, 1000, 1000], [10, 10, 10], [927, 926, 928], [138, 138, 138], [True, True, True], lam)
    assert j0[0] == j1[0] == 256 * 1000 + 146 * 11 and j1[1] == j0[1] - 256 and j1[2] == j0[2] + 256
    assert take.tolist() == [False, True, False]
    # ... and no coded child, no split, whatever the costs say
    assert not rd.tu_choice([1000], [10], [0], [4], [False], lam)[2][0]


def test_without_a_coded_child_the_children_never_win_where_the_parent_is_zero_too(draw):
    """uiCbfAny = 0: every child has r = 1 and leaves the residual as it is, so sum D1 = the residual's own energy E and J1 = 256 E + 5 lam_q8.  A parent
    without a level has D0 = E and r0 = 1: J0 = 256 E + 2 lam_q8 = J1 - 3 lam_q8 -- J1 < J0 cannot happen.  A parent WITH a level (its basis functions
    gather what no child's does) has r0 >= 4, J0 >= 256 D0 + 5 lam_q8: there J1 < J0 iff E < D0 + lam_q8 (r0 - 4) / 256, which the construction does not
    exclude; the first condition of the rule is what keeps such a TU whole.  Both halves on the draw's own TUs."""
    both_zero = parent_coded = cheaper = 0
    for bd in DEPTHS:
        d = draw[bd]
        for qp in rd.DRAW_QPS:
            lam = rd.lam_q8(qp)
            for lvl in range(4):
                s = 64 >> lvl
                items = [(k, i) for i in range(rd.DRAW_N) for k in range(85) if mr.node_geometry(k)[0] == lvl and d["per_qp"][qp][0]["cost_rd"][i, k] != rd.MARK]
                org, pred = [], []
                for k, i in items:
                    _, bx, by = mr.node_geometry(k)
                    x0, y0 = (i % rd.DRAW_CW) * 64 + bx * s, (i // rd.DRAW_CW) * 64 + by * s
                    rec = d["rec"][i, k]
                    org.append(d["cur"][y0:y0 + s, x0:x0 + s])
                    pred.append(d["planes"].block(int(rec["mvx"]), int(rec["mvy"]), x0, y0, s).astype(np.int64))
                detail = {}
                rd.node_records(np.stack(org), np.stack(pred), bd, qp, [0] * len(items), detail)
                none = ~detail["any1"]
                zero = none & ~detail["cbf0"]
                assert (detail["J1"][zero] - detail["J0"][zero] == 3 * lam).all()
                assert (detail["r0"][none & detail["cbf0"]] >= 4).all() and not detail["take"][none].any()
                both_zero += int(zero.sum())
                parent_coded += int((none & detail["cbf0"]).sum())
                cheaper += int((none & detail["cbf0"] & (detail["J1"] < detail["J0"])).sum())
    assert both_zero > 100 and parent_coded > 0
    print(f"TUs without a coded child: {both_zero} with a zero parent, {parent_coded} with a coded parent, of which {cheaper} have J1 < J0")


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", DEPTHS)
def test_the_draw_exercises_every_branch_at_every_level(draw, bd):
    d = draw[bd]
    assert d["ref"].shape == (rd.DRAW_H, rd.DRAW_W) == (152, 168) and rd.DRAW_W % 64 and rd.DRAW_H % 64 and rd.DRAW_W // 64 == 2 and rd.DRAW_H // 64 == 2
    assert d["cur"].max() == (1 << bd) - 1 and d["cur"].min() == 0
    if bd > 8:
        assert len(np.unique(d["cur"] & ((1 << (bd - 8)) - 1))) == 1 << (bd - 8)        # the low bits are in use
    total = {k: [0] * 4 for k in ("taken", "not_taken", "cbf0", "cbf1", "clipped")}
    for qp in rd.DRAW_QPS:
        for k, v in d["per_qp"][qp][1].n.items():
            total[k] = [a + b for a, b in zip(total[k], v)]
    assert all(v >= 8 for counts in total.values() for v in counts), total


@pytest.mark.parametrize("bd", DEPTHS)
def test_flag_bits_0_and_1_are_the_skip_stages_on_every_node_of_the_draw(draw, bd):
    d = draw[bd]
    for qp in rd.DRAW_QPS:
        got = d["per_qp"][qp][0]
        exp = sk.expected(d["cur"], d["ref"], rd.DRAW_W, rd.DRAW_H, bd, qp, d["rec"], 8, planes=d["planes"])
        assert np.array_equal(got["cost_rd"] == rd.MARK, exp["coef_max"] == sk.MARK)
        assert np.array_equal(got["flags"] & 3, exp["flags"]) and np.array_equal(got["mvx"], exp["mvx"]) and np.array_equal(got["mvy"], exp["mvy"])
        valid = got["cost_rd"] != rd.MARK
        # bits and cost agree with each other: cost_rd = (256 dist + lam_q8 bits) >> 8 wherever neither saturates
        plain = valid & (got["bits"] < 65535)
        assert np.array_equal(got["cost_rd"][plain], (256 * got["dist"][plain].astype(np.int64) + rd.lam_q8(qp) * got["bits"][plain].astype(np.int64)) >> 8)
        assert np.array_equal((got["flags"][valid] & rd.TU_SPLIT) != 0, got["tu_split"][valid] != 0)
        assert (got["tu_split"][:, 1:] <= 1).all()                        # only the 64x64 node has more than one depth-0 TU
        invalid = got[~valid]
        assert all(tuple(r) == rd.INVALID for r in invalid[:50])


def test_the_three_kinds_of_side_bits(draw):
    d = draw[8]
    qp = 27
    lam = rd.lam_q8(qp)
    base = d["per_qp"][qp][0]
    assert rd.merge_side_bits([0, 1, 2, 3, 4]).tolist() == [1, 2, 3, 4, 4]
    # the same vectors as explicit records: without predictor records the exp-Golomb bits of the vector, with them the record's bits; a marker predictor
    # record makes the node invalid
    q = np.zeros(d["rec"].shape, rd.capi.MOTION_QPEL_DTYPE)
    for f in ("cost_best", "mvx", "mvy"):
        q[f] = d["rec"][f]
    _, mvp = rd.draw_records(rd.EXPLICIT, 9, 8, with_mvp=True)
    plain = rd.expected(d["cur"], d["ref"], rd.DRAW_W, rd.DRAW_H, 8, qp, q, rd.EXPLICIT, 8, planes=d["planes"])
    priced = rd.expected(d["cur"], d["ref"], rd.DRAW_W, rd.DRAW_H, 8, qp, q, rd.EXPLICIT, 8, mvp=mvp, planes=d["planes"])
    valid = base["cost_rd"] != rd.MARK
    assert np.array_equal(plain["cost_rd"] != rd.MARK, valid) and np.array_equal(priced["cost_rd"] != rd.MARK, valid & (mvp["idx"] != 255))
    assert (valid & (mvp["idx"] == 255)).any()
    for out, side in ((plain, rd.explicit_side_bits(q["mvx"], q["mvy"])), (priced, mvp["bits"].astype(np.int64))):
        ok = out["cost_rd"] != rd.MARK
        assert np.array_equal(out["dist"][ok], base["dist"][ok]) and np.array_equal(out["flags"][ok], base["flags"][ok])
        delta = out["bits"][ok].astype(np.int64) - base["bits"][ok].astype(np.int64)
        assert np.array_equal(delta, side[ok] - rd.merge_side_bits(d["rec"]["idx"])[ok])
        j = 256 * out["dist"][ok].astype(np.int64) + lam * out["bits"][ok].astype(np.int64)
        assert np.array_equal(out["cost_rd"][ok], j >> 8)
