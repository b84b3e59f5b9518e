"""The restatement of the zero-residual stage (tests/motion_skip_ref.py) held to the reference's own forward transform (tests/golden/ref_transform.npz,
written by tests/quality/gen_transform_golden.py from calls into xTrMxN), to closed-form cases and to its own definition -- without a GPU.  The GPU test
(tests/test_gpu_motion_skip.py) compares the kernels with this restatement, so what is pinned here is what the kernels are held to.  Pinned HERE: the
transform, its matrices and g_quantScales.  The formula around the scales -- qbits, per / rem, the two offsets -- is compared below only with itself
(a loop, a search); tests/test_motion_skip_quant_pin.py pins it to the reference's own quantiser (tests/golden/ref_quant.npz)."""
import os

import numpy as np
import pytest

import motion_merge_cases as mc
import motion_merge_ref as mg
import motion_refine_ref as mr
import motion_skip_ref as sk
import p_tree_ref as tr
from fasthevc_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_transform.npz")
SIZES, DEPTHS = (8, 16, 32), (8, 10, 12)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_restated_matrices_and_scales_are_the_recorded_ones(golden):
    assert tuple(golden["sizes"]) == SIZES and tuple(golden["depths"]) == DEPTHS
    for n in SIZES:
        assert np.array_equal(sk.matrix(n), golden[f"matrix{n}"]), n
    assert tuple(int(v) for v in golden["quant_scales"]) == sk.QUANT_SCALES
    # the smaller matrices are rows of the larger ones
    assert np.array_equal(sk.matrix(16), sk.matrix(32)[::2, :16]) and np.array_equal(sk.matrix(8), sk.matrix(32)[::4, :8])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_the_restatement_equals_the_reference_for_every_coefficient(golden, n, bd):
    blocks, coefs = golden[f"in_{n}_{bd}"], golden[f"coef_{n}_{bd}"]
    top = (1 << bd) - 1
    assert len(blocks) >= 13 and np.abs(blocks).max() == top
    # the cases the file promises: constants, checkerboards, stripes, corner impulses
    flat = {tuple(np.unique(b)) for b in blocks}
    assert {(top,), (-top,), (-top, top)} <= flat and sum(1 for b in blocks if np.count_nonzero(b) == 1) == 4
    for i, (b, c) in enumerate(zip(blocks, coefs)):
        got = sk.forward(b, bd)
        assert np.array_equal(got, c), (n, bd, i, np.argwhere(got != c)[:5])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bd", DEPTHS)
def test_sixteen_bit_intermediates_hold_every_value(golden, n, bd):
    """the largest possible magnitude behind either stage, from the recorded matrices' absolute row sums: what lets the kernel keep 16-bit intermediates"""
    m = golden[f"matrix{n}"].astype(np.int64)
    rows = np.abs(m).sum(axis=1)
    s1, s2 = sk.shifts(n, bd)
    first = (int(rows.max()) * ((1 << bd) - 1) + (1 << (s1 - 1))) >> s1
    second = (int(rows.max()) * first + (1 << (s2 - 1))) >> s2
    assert int(rows.max()) == 64 * n and first <= 32767 and second <= 32767, (n, bd, first, second)
    # ... and the bound is reached, by the constant block: the figures are no loose estimate
    tmp, out = sk.forward(np.full((n, n), (1 << bd) - 1), bd, stages=True)
    assert int(np.abs(tmp).max()) == first and int(np.abs(out).max()) == second
    # the negative side: an arithmetic shift rounds towards minus infinity, one more in magnitude at most
    tmp, out = sk.forward(np.full((n, n), -((1 << bd) - 1)), bd, stages=True)
    assert int(np.abs(tmp).max()) <= first + 1 <= 32768 and int(np.abs(out).max()) <= second + 1 <= 32768 and tmp.min() >= -32768 and out.min() >= -32768


def test_records_equal_a_per_coefficient_loop_and_bit_1_implies_bit_0(golden):
    rng = np.random.default_rng(5)
    seen = set()
    for bd in DEPTHS:
        for s in (8, 16, 32, 64):
            for amp in (1, 3, 40, (1 << bd) - 1):
                res = rng.integers(-amp, amp + 1, size=(s, s))
                for qp in (0, 17, 22, 37, 51):
                    r = sk.node_record(res, bd, qp, (3, -4))
                    assert r == sk.node_record_loop(res, bd, qp, (3, -4)), (bd, s, amp, qp)
                    assert not (r[3] & sk.ZERO_HALF) or (r[3] & sk.ZERO_PLAIN)
                    assert (r[2] == 0) == bool(r[3] & sk.ZERO_PLAIN) and (r[1] == 0) == (r[2] == 0) and r[2] <= s * s and r[4:] == (0, 3, -4)
                    seen.add(r[3])
    assert seen == {0, 1, 3}


@pytest.mark.parametrize("bd", DEPTHS)
def test_thresholds_from_the_formula_equal_a_search(bd):
    for n in SIZES:
        for qp in range(52):
            scale, qbits, add_plain, add_half = sk.quant(n, bd, qp)
            assert 16 <= qbits <= 26 and add_plain == (85 << qbits) >> 9 and add_plain < add_half
            for half, add in ((False, add_plain), (True, add_half)):
                t = sk.first_nonzero(n, bd, qp, half)
                lo, hi = 0, 1 << 20                 # bisection: the level grows with |c|
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    lo, hi = (lo, mid) if sk.level(mid, scale, qbits, add) >= 1 else (mid, hi)
                assert hi == t and sk.level(t, scale, qbits, add) == 1 and sk.level(t - 1, scale, qbits, add) == 0, (n, qp, half)
            # the dead zone is the wider one: what RDOQ would start from zero is zero under the plain offset too
            assert sk.first_nonzero(n, bd, qp, True) <= sk.first_nonzero(n, bd, qp, False)


# ---- constructed pictures ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,fx,fy,mv", mc.HALF_CASES)
def test_a_half_sample_picture_leaves_no_residual(oracle, bd, fx, fy, mv):
    case = mc.half_sample_case(bd, fx, fy, mv)
    cur_flat = np.ascontiguousarray(case["cur"].astype(np.int16)).reshape(-1)
    merge = mg.expected(oracle, cur_flat, 0, mc.HALF_W, case["ref"], mc.HALF_W, mc.HALF_H, bd, mc.HALF_QP, case["refined"], 8, planes=case["planes"])
    inherited = merge["src"] != mg.ZERO
    assert inherited.sum() == 6 * 85 - 4
    got = sk.expected(case["cur"], case["ref"], mc.HALF_W, mc.HALF_H, bd, 22, merge, 8, planes=case["planes"])
    assert (got["coef_max"][inherited] == 0).all() and (got["coef_max"][~inherited] > 0).all()
    # coef_max == 0 is zero under both offsets at every QP
    for n in SIZES:
        for qp in range(52):
            scale, qbits, add_plain, add_half = sk.quant(n, bd, qp)
            assert sk.level(0, scale, qbits, add_plain) == 0 and sk.level(0, scale, qbits, add_half) == 0
    for qp in (0, 51):
        got = sk.expected(case["cur"], case["ref"], mc.HALF_W, mc.HALF_H, bd, qp, merge, 8, planes=case["planes"])
        assert (got["flags"][inherited] == 3).all() and (got["level_sum"][inherited] == 0).all()


def test_two_motions_leave_a_residual_astride_the_boundary(oracle):
    case = mc.two_motion_case(oracle)
    cur, ref = (p.astype(np.int64) for p in mc.pictures())
    got = sk.expected(cur, ref, mc.W, mc.H, 8, 22, case["merge"], mc.RANGE)
    # CTU 1's nodes along its left edge have CTU 0's motion as their L candidate: those that took a vector other than V2 are far from zero
    q2 = (4 * mc.V2[0], 4 * mc.V2[1])
    wrong = (case["merge"]["mvx"][1] != q2[0]) | (case["merge"]["mvy"][1] != q2[1])
    assert wrong[0] and wrong.sum() >= 4 and (got["flags"][1][wrong] == 0).all() and (got["nonzero"][1][wrong] > 0).all()
    assert got["nonzero"][1, 0] > 1000
    # ... and every node that inherited its CTU's own vector is exactly zero
    right = ~wrong
    assert right.any() and (got["coef_max"][1][right] == 0).all() and (got["flags"][1][right] == 3).all()
    assert got["flags"][2, 0] == 3 and got["coef_max"][2, 0] == 0


@pytest.mark.parametrize("bd,d", sk.FLAT_CASES)
def test_a_flat_offset_has_one_coefficient_and_flips_once_per_bit(bd, d):
    exp = sk.flat_offset_expectation(bd, d)
    for lvl in range(4):                             # each bit flips inside the QP range, once, and bit 1 later than bit 0
        plain, half = exp[lvl]
        assert 0 < len(half) < len(plain) < 52 and plain == set(range(min(plain), 52)) and half == set(range(min(half), 52)), (lvl, exp[lvl])
    assert min(exp[0][0]) == min(exp[1][0]) > min(exp[2][0]) > min(exp[3][0])          # a larger TU has fewer qbits: it stays non-zero longer
    # the closed form: the DC coefficient is d << (15 - bd), nothing else is non-zero
    for s in (8, 16, 32, 64):
        c = sk.coefficients(np.full((s, s), d), bd)
        assert np.count_nonzero(c) == (4 if s == 64 else 1) and int(c.max()) == d << (15 - bd)
    # the restatement over a picture agrees with the thresholds
    w, h = 192, 64
    ref = np.full((h, w), 1 << (bd - 1), np.int64)
    merge = np.zeros((3, 85), capi.MOTION_MERGE_DTYPE)
    merge["cost_best"] = 7
    planes = mr.Planes(ref, bd, 12)
    for qp in (0, min(exp[3][0]) - 1, min(exp[3][0]), min(exp[0][1]) - 1, min(exp[0][1]), 51):
        got = sk.expected(ref + d, ref, w, h, bd, qp, merge, 4, planes=planes)
        for k in range(85):
            lvl = tr.level(k)
            assert (got["flags"][:, k] == ((1 if qp in exp[lvl][0] else 0) | (2 if qp in exp[lvl][1] else 0))).all(), (qp, k)


# ---- the tree rule ------------------------------------------------------------------------------------------------------------------------------------------

W, H = 200, 136


def test_tree_rule_against_the_merge_tree():
    rng = np.random.default_rng(823)
    shapes = tr.random_shapes(rng, 2, 12)
    merge = mg.random_merge(rng, shapes)
    skip = sk.random_skip(rng, (2, 12, 85))
    for ctu, f in zip((0, 1, 2, 4), (0, 1, 2, 3)):
        shapes["cost_best"][0, ctu, 0], merge["cost_best"][0, ctu, 0], skip["flags"][0, ctu, 0] = 40000, 39000, f
    for rule in (None, tr.random_rule(rng)):
        base = mg.tree_select(shapes, merge, W, H, rule=rule)
        zero = sk.tree_select(shapes, merge, skip, 0, W, H, rule=rule)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base, zero))          # skip_mask 0 is the merge tree
        merged = (base[0]["flags"] & mg.MERGED) != 0
        seen = sk.flag_coverage(skip, merged)
        assert all(seen[l] == {0, 1, 2, 3} for l in range(3)), seen               # at every level, nodes with and without each masked bit
        for mask in (1, 2, 3):
            rec, dmin, dmax = sk.tree_select(shapes, merge, skip, mask, W, H, rule=rule)
            f = rec["flags"]
            skipped = (f & sk.SKIPPED) != 0
            assert skipped.any() and not (skipped & ~merged).any() and not skipped[..., 21:].any()        # bit 7 only with bit 6, only at levels 0..2
            want = merged & ((skip["flags"] & mask) != 0)
            want[..., 21:] = False
            assert np.array_equal(skipped, want)
            assert (rec["cost_tree"][skipped] == rec["cost_own"][skipped]).all() and ((f[skipped] & 3) == tr.STOP_SURE).all()
            assert (dmin <= dmax).all()
            # own costs and the leaves are the merge tree's: only trees and decisions at and above a skip move
            assert (rec["cost_own"] == base[0]["cost_own"]).all() and rec[..., 21:].tobytes() == base[0][..., 21:].tobytes()


def test_a_skipped_root_is_not_descended():
    shapes, merge, skip = sk.root_skip_case()
    for mask, depth in ((0, 1), (1, 1), (2, 0), (3, 0)):
        rec, dmin, dmax = sk.tree_select(shapes, merge, skip, mask, 64, 64)
        assert rec["cost_kids"][0, 0, 0] == 40 < rec["cost_own"][0, 0, 0] == 90000
        assert (dmax == depth).all() and (dmin == depth).all()
        assert rec["cost_tree"][0, 0, 0] == (90000 if depth == 0 else 40) and bool(rec["flags"][0, 0, 0] & sk.SKIPPED) == (depth == 0)
        assert bool(rec["flags"][0, 0, 0] & tr.STOP_SURE) == (depth == 0) and bool(rec["flags"][0, 0, 0] & tr.SPLIT_SURE) == (depth != 0)
