"""The CPU oracle reads nothing outside the picture rectangle for its value: every oracle entry point the GPU layout tests
(tests/test_gpu_layouts.py) use as their reference gives byte-identical results on a zero-margin plane in HM's layout and on planes
whose margins, stride padding and surroundings are poison (frames.guarded_plane), with an odd stride and a moved origin.  The golden
tests pin the oracle to the reference on zero or replicated margins only; this file is what lets the oracle serve on any layout."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as op
from fasthevc_amd import capi, frames, weights

W, H = 200, 136   # partial CTUs in both directions, width not a multiple of 16
LAYOUTS = [dict(extra_stride=3, shift=5, poison=11), dict(extra_stride=1, shift=1, frame_gap=0, poison=12, margin=3)]


def _pictures(bd):
    ys = frames.pan_clip(W, H, 2, seed=31 + bd, v_structure=5, v_noise=-3)
    rng = np.random.default_rng(bd)
    return [(y.astype(np.int16) << (bd - 8)) | rng.integers(0, 1 << (bd - 8), size=y.shape).astype(np.int16) for y in ys]


def _planes(bd):
    """the same two pictures (a pan pair) as a clean HM plane and under both poisoned layouts: [(flat, origin, stride, frame_stride)]"""
    pics = _pictures(bd)
    return [frames.guarded_plane(pics, bd, poison=None)] + [frames.guarded_plane(pics, bd, **kw) for kw in LAYOUTS]


def _same_on_every_layout(bd, fn):
    planes = _planes(bd)
    assert planes[1][2] % 2 == 1 and (planes[1][0].ctypes.data + 2 * planes[1][1]) % 4 != 0   # odd stride, origin off 4-byte alignment
    results = [fn(*p) for p in planes]
    for k, r in enumerate(results[1:]):
        assert len(r) == len(results[0])
        for a, b in zip(results[0], r):
            assert a.tobytes() == b.tobytes(), f"layout {k + 1} differs from the zero-margin plane"
    return results[0]


@pytest.mark.parametrize("bd", [8, 10])
def test_depth_classifier_and_source_hadamard(oracle, bd):
    w = weights.random_weights(4)
    n = 4 * 3

    def run(flat, org, stride, fs):
        depth, logits, had = np.zeros(n * 256, np.uint8), np.zeros(n * 42, np.int32), np.zeros(n, np.int32)
        oracle.fho_predict_frame(op.weights_from_arrays(w), op.ptr(flat, org), stride, W, H, bd, 30, depth, C.c_void_p(logits.ctypes.data))
        oracle.fho_frame_src_hadamard(op.ptr(flat, org), stride, W, H, had)
        return depth, logits, had

    depth, _, had = _same_on_every_layout(bd, run)
    assert len(np.unique(depth)) >= 2 and had.any()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("widths,depth", [((32, 64, 128), 1), ((23, 46, 92), 2)])
def test_family_classifier(oracle, bd, widths, depth):
    fam = weights.random_family(widths, depth, seed=bd)
    n = 4 * 3

    def run(flat, org, stride, fs):
        d, logits = np.zeros(n * 256, np.uint8), np.zeros(n * 42, np.int32)
        oracle.fho_predict_frame_family(C.byref(op.family_from_arrays(fam)), op.ptr(flat, org + fs), stride, W, H, bd, 27, d.ctypes.data, logits.ctypes.data)
        return d, logits

    _same_on_every_layout(bd, run)


@pytest.mark.parametrize("bd", [8, 10])
def test_first_pass_best_all_modes_and_candidates(oracle, bd):
    sl = oracle.fho_lambda_intra(33, bd) ** 0.5
    oracle.fho_first_pass_candidates_ctu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]

    def run(flat, org, stride, fs):
        best = np.zeros((12, 85), capi.NODE_DTYPE)
        for c in range(12):
            oracle.fho_first_pass_ctu(op.ptr(flat, org), stride, W, H, c % 4, c // 4, bd, sl, best[c].ctypes.data_as(C.POINTER(op.NodeCost)))
        sat = np.zeros((4, 85, 35), np.uint32)
        cand = np.zeros((4, 85, 8), np.uint8)
        node = op.NodeCost()
        for i, c in enumerate((0, 3, 8, 11)):   # first, right-most, bottom-most, corner
            idx = 0
            for lvl in range(4):
                nn, cnt = 64 >> lvl, 1 << lvl
                for by in range(cnt):
                    for bx in range(cnt):
                        x0, y0 = (c % 4) * 64 + bx * nn, (c // 4) * 64 + by * nn
                        if x0 + nn <= W and y0 + nn <= H:
                            oracle.fho_first_pass_node(op.ptr(flat, org), stride, W, H, x0, y0, nn, bd, sl, C.byref(node), C.c_void_p(sat[i, idx].ctypes.data))
                        idx += 1
            oracle.fho_first_pass_candidates_ctu(op.ptr(flat, org), stride, W, H, c % 4, c // 4, bd, C.c_double(sl), 8, cand[i].ctypes.data)
        return best, sat, cand

    best, sat, _ = _same_on_every_layout(bd, run)
    assert (best["mode"] == 255).any() and (best["mode"] < 35).any() and sat.any()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("sad,rng", [(0, 4), (1, 8), (1, 33)])
def test_motion_search(oracle, bd, sad, rng):
    sl = oracle.fho_lambda_intra(35, bd) ** 0.5

    def run(flat, org, stride, fs):
        out = np.zeros((12, 85), capi.MOTION_DTYPE)
        for c in range(12):
            oracle.fho_motion_ctu_dist(op.ptr(flat, org + fs), stride, op.ptr(flat, org), stride, W, H, c % 4, c // 4, bd, rng, C.c_double(sl), sad,
                                       C.c_void_p(out[c].ctypes.data))
        return (out,)

    (out,) = _same_on_every_layout(bd, run)
    assert (out["mvx"] != 0).any()


@pytest.mark.parametrize("bd", [8, 10])
def test_preanalysis(oracle, bd):
    def run(flat, org, stride, fs):
        res = []
        for d in range(4):
            p = 64 >> d
            act = np.zeros(((H + p - 1) // p) * ((W + p - 1) // p))
            avg = oracle.fho_preanalyze_layer(op.ptr(flat, org), stride, W, H, p, act)
            res += [act, np.array([avg])]
        return res

    _same_on_every_layout(bd, run)


def test_guarded_plane_layout_and_poison():
    """the builder itself: HM's layout when nothing is asked for, every non-picture sample poisoned, alignment moved by exactly `shift`"""
    y = frames.texture16_luma(W, H, seed=3)
    ref, org0, stride0 = frames.to_pel_plane(y, 10)
    flat, org, stride, fs = frames.guarded_plane(y.astype(np.int16) << 2, 10, poison=None)
    assert stride == stride0 and fs == ref.size and flat.ctypes.data % 64 == 0 and (flat.ctypes.data + 2 * org) % 16 == 0
    assert np.array_equal(flat[org - org0:org - org0 + ref.size], ref.reshape(-1)) and not flat[:org - org0].any()
    for dtype, bd, pics in ((np.int16, 10, [y.astype(np.int16) << 2] * 3), (np.uint8, 8, [y] * 3)):
        for shift, extra, gap in ((0, 0, 0), (1, 3, 5), (7, 8, 13)):
            a, org, stride, fs = frames.guarded_plane(pics, bd, dtype, extra_stride=extra, shift=shift, frame_gap=gap, poison=5)
            b = frames.guarded_plane(pics, bd, dtype, extra_stride=extra, shift=shift, frame_gap=gap, poison=6)[0]
            item = np.dtype(dtype).itemsize
            assert (a.ctypes.data + item * org) % 64 == ((frames.HM_MARGIN * stride + frames.HM_MARGIN + shift) * item) % 64
            assert stride == W + 160 + extra and fs == (H + 160) * stride + gap
            inside = np.zeros(a.size, bool)
            for f in range(3):
                idx = org + f * fs + np.arange(H)[:, None] * stride + np.arange(W)[None, :]
                assert np.array_equal(a[idx], pics[f]) and np.array_equal(b[idx], pics[f])
                inside[idx] = True
            first, last = org - frames.HM_MARGIN * stride - frames.HM_MARGIN, org + 2 * fs + (H - 1) * stride + W
            assert first * item >= 4096 and (a.size - last) * item >= 4096            # the guard zones
            out_a, out_b = a[~inside], b[~inside]
            assert (out_a != out_b).mean() > 0.5 and len(np.unique(out_a)) > 100       # poison, and another one per seed
            want = (0, 255) if dtype == np.uint8 else (-32768, 32767, -1, 1023, 1024)
            assert all((out_a == v).mean() > 0.05 for v in want)
            # the samples that touch the picture: the column left and right of it and the rows above and below are not all zero
            for f in range(3):
                o = org + f * fs
                assert a[o - 1:o - 1 + H * stride:stride].any() and a[o + W:o + W + H * stride:stride].any()
                assert a[o - stride:o - stride + W].any() and a[o + H * stride:o + H * stride + W].any()
