"""The CPU oracle (oracle/fhevc_oracle.c) at bit depths 9 to 12 and on full-swing samples, against what the reference's own
functions returned (tests/golden/ref_bit_depths.npz, oracle/gen_golden.py: bit_depths_golden).  The inputs are regenerated
from the seeds of oracle/bd_cases.py; the GPU kernels are held to this oracle in tests/test_gpu_bit_depths.py."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import bd_cases as bc
from oracle import oracle_py as op
from fasthevc_amd import frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_bit_depths.npz"))


def test_native_planes_reach_both_ends_of_the_range():
    for bd in (9, 10, 11, 12):
        buf, org, stride = frames.native_pel_plane(frames.texture16_luma(200, 136), bd, seed=bd)
        m = org % stride
        pic = buf[m:m + 136, m:m + 200]
        assert pic.min() == 0 and pic.max() == (1 << bd) - 1 and stride == 200 + 2 * frames.HM_MARGIN
        assert len(np.unique(pic & ((1 << (bd - 8)) - 1))) == 1 << (bd - 8)  # the low bits are populated
        assert not buf[:m].any() and not buf[:, :m].any()


def test_satd_matches_reference(oracle, g):
    meta = g["satd_meta"]
    assert len(meta) == len(bc.SATD_BIT_DEPTHS) * len(bc.SATD_SHAPES) * len(bc.SATD_KINDS)
    peak = 0
    for i, (bd, w, h, rep) in enumerate(meta):
        bd, w, h, rep = int(bd), int(w), int(h), int(rep)
        a, b = bc.satd_pair(bd, w, h, bc.SATD_KINDS[rep], rep)
        got = oracle.fho_satd(op.ptr(a), 64, op.ptr(b), 64, w, h, bd)
        assert got == int(g["satd_gethads"][i]), (bd, w, h, bc.SATD_KINDS[rep])
        if g["satd_calchad"][i] != 0xFFFFFFFF:
            assert got == int(g["satd_calchad"][i]), (bd, w, h, bc.SATD_KINDS[rep])
        if bc.SATD_KINDS[rep] == "basis" and w % 8 == 0 and h % 8 == 0:
            peak = max(peak, got)
    # a full-swing basis pattern puts 64 (2^bd - 1) into one coefficient of every 8x8; 64 blocks of 64x64 at 12 bit, >> (bd - 8)
    assert peak == (((64 * 4095 + 2) >> 2) * 64) >> 4


def test_fill_reference_samples(oracle, g):
    for bd in bc.INTRA_BIT_DEPTHS:
        for n in bc.INTRA_SIZES:
            exp = g[f"fill_n{n}_bd{bd}"]
            for rep in range(bc.FILL_REPS):
                pic, flags = bc.fill_case(bd, n, rep)
                side = pic.shape[1]
                line = np.zeros(4 * n + 1, np.int16)
                oracle.fho_fill_ref_flags(op.ptr(pic.reshape(-1), 4 * side + 4), side, flags, n, bd, line)
                assert np.array_equal(line, exp[rep]), (bd, n, rep)


def test_intra_predictors(oracle, g):
    for bd in bc.INTRA_BIT_DEPTHS:
        for n in bc.INTRA_SIZES:
            for kind in ("sat", "flat"):
                line = bc.pred_line(bd, n, kind)
                exp = g[f"pred_{kind}_n{n}_bd{bd}"]
                if kind == "sat":
                    assert line.min() == 0 and line.max() == (1 << bd) - 1
                for m in range(35):
                    pred = np.zeros(n * n, np.int16)
                    oracle.fho_pred_intra(line, line, n, m, bd, pred)
                    assert np.array_equal(pred.reshape(n, n), exp[m]), (bd, n, kind, m)


def test_reference_lines_from_the_references_own_init_intra_pattern(oracle, g):
    """Unfiltered and smoothed lines of live CUs at 9 and 11 bit; the strong (bilinear) smoothing is decided by 2^(bd - 5),
    16 at 9 bit and 64 at 11 bit, and the goldens hold 32x32 / 64x64 lines on both sides of it."""
    near = {}
    for k, (content, w, h, bd, _qp, _ctus) in enumerate(bc.INTRA_LINE_CASES):
        buf, org, stride = bc.intra_line_plane(content, w, h, bd)
        unf_all, flt_all = g[f"lines_unf{k}"], g[f"lines_flt{k}"]
        off = 0
        strong = plain_only = 0
        for (c, depth, x0, y0, n) in g[f"lines_meta{k}"]:
            n = int(n)
            ln = 4 * n + 1
            unf, flt = unf_all[off:off + ln], flt_all[off:off + ln]
            off += ln
            line, out = np.zeros(ln, np.int16), np.zeros(ln, np.int16)
            oracle.fho_fill_ref(op.ptr(buf.reshape(-1), org), stride, w, h, int(x0), int(y0), n, bd, line)
            assert np.array_equal(line, unf), ("unfiltered", bd, int(c), int(depth), int(x0), int(y0))
            oracle.fho_filter_ref(line, n, bd, 1, out)
            assert np.array_equal(out, flt), ("filtered", bd, int(c), int(depth), int(x0), int(y0))
            if n >= 32:
                l = line.astype(int)
                dev = max(abs(l[0] + l[2 * n] - 2 * l[n]), abs(l[2 * n] + l[4 * n] - 2 * l[3 * n]))
                plain = np.zeros(ln, np.int16)
                oracle.fho_filter_ref(line, n, bd, 0, plain)
                if np.array_equal(plain, out):
                    plain_only += 1
                else:
                    strong += 1
                thr = 1 << (bd - 5)
                if thr // 2 <= dev < 2 * thr:  # within a factor two of this depth's threshold: the 10-bit one (32) decides otherwise
                    near[bd] = near.get(bd, 0) + 1
        assert off == unf_all.size
        assert strong > 0 and plain_only > 0, (bd, strong, plain_only)
    assert near.get(9, 0) > 0 and near.get(11, 0) > 0, near


def _layer_sizes(w, h, depth):
    return [((w + (64 >> d) - 1) // (64 >> d)) * ((h + (64 >> d) - 1) // (64 >> d)) for d in range(depth)]


def test_preanalysis_and_aq_qp(oracle, g):
    clipped = set()
    for k, (content, w, h, bd, depth) in enumerate(bc.PREANALYZE_CASES):
        buf, org, stride = bc.preanalyze_plane(content, w, h, bd)
        if content != "hetero":
            m = org % stride
            assert buf[m:m + h, m:m + w].max() == (1 << bd) - 1
        acts, avgs = [], []
        for d, n in enumerate(_layer_sizes(w, h, depth)):
            a = np.zeros(n)
            avgs.append(oracle.fho_preanalyze_layer(op.ptr(buf.reshape(-1), org), stride, w, h, 64 >> d, a))
            acts.append(a)
        act = np.concatenate(acts)
        assert act.tobytes() == g[f"pre_act{k}"].tobytes(), (content, bd)  # bit patterns of the doubles
        assert np.array(avgs).tobytes() == g[f"pre_avg{k}"].tobytes(), (content, bd)
        off = np.cumsum([0] + _layer_sizes(w, h, depth))
        for s, (range_, qp) in enumerate(bc.AQ_SETTINGS):
            exp = g[f"pre_qp{k}_{s}"].astype(int)
            got = np.array([oracle.fho_aq_qp(act[i], avgs[int(np.searchsorted(off, i, "right")) - 1], range_, qp, 6 * (bd - 8))
                            for i in range(act.size)])
            assert np.array_equal(got, exp), (content, bd, range_, qp)
            if (exp == -6 * (bd - 8)).any():
                clipped.add(bd)
    assert {9, 11} <= clipped  # the lower clip at -qp_bd_offset (6 and 18) is reached


def test_motion_search_sad_mode_equals_the_references_xPatternSearch(oracle, g):
    W, H = 416, 240
    checked = 0
    for k, (bd, qp, rng, content, seed, ctus) in enumerate(bc.PATTERN_CASES):
        cur, ref, stride = bc.pattern_planes(bd, content, seed)
        if content == "pan":
            assert cur.min() == 0 and cur.max() == (1 << bd) - 1
        sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
        out = np.zeros(85, [("zero", np.uint32), ("best", np.uint32), ("cost", np.uint32), ("mvx", np.int16), ("mvy", np.int16)])
        for ci, c in enumerate(ctus):
            oracle.fho_motion_ctu_dist(C.c_void_p(cur.ctypes.data), stride, C.c_void_p(ref.ctypes.data), stride, W, H, c % 7, c // 7, bd, rng,
                                       C.c_double(sl), 1, C.c_void_p(out.ctypes.data))
            exp = g[f"ps_nodes{k}"][ci]
            valid = exp[:, 3] >= 0
            assert valid.sum() > 0 and (out["cost"][~valid] == 0xFFFFFFFF).all()
            assert np.array_equal(out["mvx"][valid], exp[valid, 0]) and np.array_equal(out["mvy"][valid], exp[valid, 1]), (k, c)
            assert np.array_equal(out["best"][valid], exp[valid, 2].astype(np.uint32)), (k, c)
            assert np.array_equal(out["cost"][valid], exp[valid, 3].astype(np.uint32)), (k, c)
            checked += int(valid.sum())
    assert checked > 700
