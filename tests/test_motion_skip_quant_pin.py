"""The quantiser and the two zero bits of the zero-residual stage held to the reference's own quantiser -- without a GPU, from tests/golden/ref_quant.npz
alone (written by tests/quality/gen_quant_golden.py from calls into TComTrQuant::xQuant and xRateDistOptQuant on a live CU, QpParam by the reference's own
constructor).  What is pinned: motion_skip_ref.quant() -- qbits, the per / rem split of qp + 6 (bd - 8), add_plain = 85 << (qbits - 9) --, first_nonzero()
for both offsets, and node_record() on real predicted nodes: coef_max, level_sum, nonzero and bit 0 for equality, bit 1 as the sufficient condition it is
(bit 1 set -> the reference's RDOQ codes nothing).  tests/test_gpu_motion_skip_quant_pin.py holds the kernel to the same file."""
import numpy as np
import pytest

import motion_refine_ref as mr
import motion_skip_quant_cases as qc
import motion_skip_ref as sk


@pytest.fixture(scope="module")
def quant_golden():
    return np.load(qc.GOLDEN)


def test_the_file_holds_the_cases_it_promises(quant_golden):
    g = quant_golden
    assert tuple(g["sizes"]) == qc.SIZES and tuple(g["depths"]) == qc.DEPTHS and tuple(g["node_qps"]) == qc.NODE_QPS and tuple(g["ranges"]) == qc.RANGES
    assert g["thr_levels"].shape == (3, 3, 52, qc.K) and g["thr_random"].shape == (qc.NUM_RANDOM,) and qc.NUM_RANDOM >= 200
    r = g["thr_random"].astype(np.int64)
    assert r.min() < -30000 and r.max() > 30000 and len(np.unique(r >> 12)) == 16          # over the 16-bit range
    assert all(a.dtype.kind in "iu" for a in g.values())                                   # integers only
    fixed = g["thr_special"][..., 12:]
    assert (fixed == np.array(qc.FIXED)).all()


def threshold_case(g, i, j, qp):
    """-> (coefficients [K] int64, recorded levels [K] int64, RDOQ non-zero map [K] bool)"""
    c = np.concatenate([g["thr_special"][i, j, qp], g["thr_random"].astype(np.int32)]).astype(np.int64)
    return c, g["thr_levels"][i, j, qp].astype(np.int64), np.unpackbits(g["thr_rdoq_nonzero"][i, j, qp]).astype(bool)


@pytest.mark.parametrize("bd", qc.DEPTHS)
@pytest.mark.parametrize("n", qc.SIZES)
def test_levels_and_thresholds_are_the_references_at_every_qp(quant_golden, n, bd):
    g = quant_golden
    i, j = qc.SIZES.index(n), qc.DEPTHS.index(bd)
    for qp in qc.ALL_QPS:
        c, rec, hard = threshold_case(g, i, j, qp)
        scale, qbits, add_plain, add_half = sk.quant(n, bd, qp)
        # every recorded level, sign included, under the plain offset
        mine = np.array([(1 if v >= 0 else -1) * sk.level(v, scale, qbits, add_plain) for v in c.tolist()], np.int64)
        bad = mine != rec
        assert not bad.any(), (n, bd, qp, c[bad][:5].tolist(), mine[bad][:5].tolist(), rec[bad][:5].tolist())
        # uiAbsSum per block is the sum of the magnitudes
        sums = np.abs(qc.threshold_blocks(rec, n)).reshape(qc.num_blocks(n), -1).sum(axis=1)
        assert np.array_equal(sums, g["thr_abs_sum"][i, j, qp, :qc.num_blocks(n)]), (n, bd, qp)
        # the plain threshold is exactly where the recorded levels go from 0 to 1, in both signs
        t = sk.first_nonzero(n, bd, qp, False)
        for s in (1, -1):
            side = c[c * s > 0] * s
            lv = rec[c * s > 0] * s
            assert side[lv == 0].max() == t - 1 and side[lv >= 1].min() == t and (lv[side == t] == 1).all(), (n, bd, qp, s, t)
        assert (rec[c == 0] == 0).all()
        # the half threshold: below it the reference's RDOQ leaves nothing; the coefficients t - 1 of both signs are among the recorded ones
        th = sk.first_nonzero(n, bd, qp, True)
        assert th == -(-((1 << qbits) - add_half) // scale) and (c == th - 1).any() and (c == 1 - th).any() and (c == th).any()
        below = np.abs(c) < th
        assert not hard[below].any(), (n, bd, qp, th, c[below & hard][:5].tolist())
        # ... and a block RDOQ reports as empty (uiAbsSum == 0) has no non-zero position
        blocks = qc.threshold_blocks(hard.astype(np.int32), n).reshape(qc.num_blocks(n), -1)
        assert np.array_equal(~blocks.any(axis=1), g["thr_rdoq_zero"][i, j, qp, :qc.num_blocks(n)] != 0), (n, bd, qp)


def test_rdoq_keeps_coefficients_above_the_half_threshold_somewhere(quant_golden):
    """the implication above is no empty statement: at every size and bit depth RDOQ keeps recorded coefficients, and the smallest magnitude it keeps is
    never below the half threshold"""
    g = quant_golden
    for i, n in enumerate(qc.SIZES):
        for j, bd in enumerate(qc.DEPTHS):
            kept = 0
            for qp in qc.ALL_QPS:
                c, _, hard = threshold_case(g, i, j, qp)
                kept += int(hard.sum())
                assert not hard.any() or np.abs(c[hard]).min() >= sk.first_nonzero(n, bd, qp, True)
            assert kept > 1000, (n, bd, kept)


# ---- real nodes ---------------------------------------------------------------------------------------------------------------------------------------------

_NODES = {}


def node_case(g, bd):
    """per bit depth, computed once: the regenerated pictures, the stored merge records, and motion_skip_ref's records [ranges, CTUS, 85, QPs]"""
    if bd not in _NODES:
        pics = qc.pictures(bd)
        merges = np.ascontiguousarray(g[f"merge_{bd}"]).view(sk.mg.MDT).reshape(len(qc.RANGES), qc.CTUS, 85)
        mine = np.zeros((len(qc.RANGES), qc.CTUS, 85, len(qc.NODE_QPS)), sk.SDT)
        for r, R in enumerate(qc.RANGES):
            planes = mr.Planes(pics[0], bd, R + 8)
            for i, qp in enumerate(qc.NODE_QPS):
                mine[r, :, :, i] = sk.expected(pics[1], pics[0], qc.W, qc.H, bd, qp, merges[r], R, planes=planes)
        _NODES[bd] = (pics, merges, mine)
    return _NODES[bd]


@pytest.mark.parametrize("bd", qc.DEPTHS)
def test_the_regenerated_pictures_are_the_generators(quant_golden, bd):
    pics, _, _ = node_case(quant_golden, bd)
    assert qc.picture_hash(pics) == bytes(quant_golden[f"sha256_{bd}"]).hex()
    assert all(p.shape == (qc.H, qc.W) and p.min() >= 0 and p.max() < (1 << bd) for p in pics)


@pytest.mark.parametrize("bd", qc.DEPTHS)
def test_node_records_are_the_references_numbers(quant_golden, bd):
    g = quant_golden
    _, merges, mine = node_case(g, bd)
    more = 0
    for r, R in enumerate(qc.RANGES):
        ok = qc.valid(merges[r], R)
        # the merge records hold what the file promises: marked ones, ones beyond the reach, the zero vector, whole-sample and fractional vectors
        far = (np.abs(merges[r]["mvx"].astype(np.int64)) > 4 * R + 3) | (np.abs(merges[r]["mvy"].astype(np.int64)) > 4 * R + 3)
        assert (merges[r]["cost_best"] == sk.MARK).sum() >= 10 and far.sum() >= 8 and ok[:, 0].all()
        zero = ok & (merges[r]["mvx"] == 0) & (merges[r]["mvy"] == 0)
        whole = ok & (merges[r]["mvx"] % 4 == 0) & (merges[r]["mvy"] % 4 == 0)
        assert zero.sum() >= 5 and whole.sum() >= 40 and (ok & ~whole).sum() >= 20
        for i, qp in enumerate(qc.NODE_QPS):
            m = mine[r, :, :, i]
            assert np.array_equal(m["coef_max"] != sk.MARK, ok), (bd, R, qp)
            for field, rec in (("coef_max", g[f"coef_max_{bd}"][r]), ("level_sum", g[f"level_sum_{bd}"][r, :, :, i]), ("nonzero", g[f"nonzero_{bd}"][r, :, :, i])):
                bad = ok & (m[field] != rec)
                assert not bad.any(), (bd, R, qp, field, np.argwhere(bad)[:5].tolist(), m[field][bad][:5].tolist(), rec[bad][:5].tolist())
            plain_zero = g[f"level_sum_{bd}"][r, :, :, i] == 0
            assert np.array_equal(((m["flags"] & sk.ZERO_PLAIN) != 0)[ok], plain_zero[ok]), (bd, R, qp)
            half = ((m["flags"] & sk.ZERO_HALF) != 0) & ok
            hard_zero = g[f"rdoq_zero_{bd}"][r, :, :, i] != 0
            assert not (half & ~hard_zero).any(), (bd, R, qp, np.argwhere(half & ~hard_zero)[:5].tolist())      # bit 1 -> RDOQ codes nothing
            more += int((ok & ~half & hard_zero).sum())
    print(f"bit depth {bd}: RDOQ zeroed more than the half bit says on {more} node / QP pairs")


@pytest.mark.parametrize("bd", qc.DEPTHS)
def test_every_outcome_is_covered_at_every_level(quant_golden, bd):
    g = quant_golden
    _, merges, mine = node_case(g, bd)
    ok = np.stack([qc.valid(merges[r], R) for r, R in enumerate(qc.RANGES)])
    okq = np.broadcast_to(ok[..., None], mine.shape)
    level_sum = g[f"level_sum_{bd}"]
    cov = qc.coverage(level_sum == 0, (mine["flags"] & sk.ZERO_HALF) != 0, okq)
    hard = qc.coverage(level_sum == 0, g[f"rdoq_zero_{bd}"] != 0, okq)
    print(f"bit depth {bd}: per level (plain zero, plain non-zero, half bit set, half bit clear) {cov}; (.., .., RDOQ all-zero, not) {hard}")
    assert all(min(c) >= qc.MIN_PAIRS for c in cov.values()), cov
    assert all(min(c) >= qc.MIN_PAIRS for c in hard.values()), hard
    assert (level_sum[okq] >= 2).any()                        # sign hiding, off for the recorded calls, would have had levels to change
    # the 64x64 nodes (four TUs each) are compared at every QP, and no compared node is the trivial all-zero residual
    assert ok[:, :, 0].all() and (g[f"nonzero_{bd}"][:, :, 0, 0] > 0).all() and (g[f"coef_max_{bd}"][ok] > 0).all()
