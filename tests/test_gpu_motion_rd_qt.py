"""Config 4 (P slices): the RD stages with the depth count (fhevc_motion_rd_qt*, fhevc_motion_rd_pu_qt*, fhevc_p_tree_rd_qt_frame: further instances of
k_motion_rd.hip) on the MI355X, byte for byte against the restatement tests/motion_rd_qt_ref.py, which tests/test_motion_rd_qt_ref.py holds against the
two-depth restatements and hand-set numbers without a GPU.  Nothing is compared with the kernel's own output except where two launches must give the same
bytes: tu_depths 2 against the entry points without the argument, the 64x64 and 8x8 nodes across the depth counts, bands against the whole.

Pictures are the restatement's draw, 168 x 152 = 3 x 3 CTUs, ragged in both directions; the other shapes are 64 x 64, 72 x 72 and 64 x 128."""
import ctypes as C

import numpy as np
import pytest

import intra_rd_ref as ir
import motion_rd_pu_ref as pu
import motion_rd_qt_ref as qt
import motion_rd_ref as rd
import motion_refine_ref as mr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)
from test_gpu_motion_rd import Guarded, at_offset
from test_gpu_motion_rd_pu import DevInputs

pytestmark = pytest.mark.gpu

W, H, CW, CH, N = rd.DRAW_W, rd.DRAW_H, rd.DRAW_CW, rd.DRAW_CH, rd.DRAW_N
MDT, QDT, PDT, SDT, RDT, RPT = capi.MOTION_MERGE_DTYPE, capi.MOTION_QPEL_DTYPE, capi.MOTION_MVP_DTYPE, capi.SHAPE_DTYPE, capi.MOTION_RD_DTYPE, capi.MOTION_RD_PU_DTYPE
LEVEL_OF = np.array([mr.node_geometry(k)[0] for k in range(85)])
OUTER, INNER = (LEVEL_OF == 0) | (LEVEL_OF == 3), (LEVEL_OF == 1) | (LEVEL_OF == 2)
_CACHE = {}


def pictures(bd):
    """three pictures at bd bits: frame 1 (the draw's current picture, with the bumps) is predicted from frame 0, frame 2 from frame 1"""
    if ("pics", bd) not in _CACHE:
        ref, cur = qt.draw_pictures(bd)
        _CACHE[("pics", bd)] = [ref, cur, qt.draw_pictures(bd, seed=1)[1]]
    return _CACHE[("pics", bd)]


def planes_of(bd, f, max_range):
    pad = 16 if max_range <= 8 else 72
    if ("planes", bd, f, pad) not in _CACHE:
        _CACHE[("planes", bd, f, pad)] = mr.Planes(pictures(bd)[f], bd, pad)
    return _CACHE[("planes", bd, f, pad)]


def plane_batch(bd, nf, dtype=np.int16, **kw):
    return frames.guarded_plane([pictures(bd)[f % 3] for f in range(nf)], bit_depth=bd, dtype=dtype, poison=kw.pop("poison", None), **kw)


def expected_plain(bd, qp, recs, source, max_range, tud, mvp=None, rows=None):
    """recs [pairs, band CTUs, 85] -> the records of the same shape"""
    pics = pictures(bd)
    return np.stack([qt.expected(pics[f % 3], pics[(f - 1) % 3], W, H, bd, qp, recs[f - 1], source, max_range, tud, mvp=None if mvp is None else mvp[f - 1], rows=rows,
                                 planes=planes_of(bd, (f - 1) % 3, max_range)) for f in range(1, recs.shape[0] + 1)])


def expected_pu(bd, qp, mode, inps, max_range, tud, rows=None, fold_into=None):
    pics = pictures(bd)
    return np.stack([qt.expected_pu(pics[f % 3], pics[(f - 1) % 3], W, H, bd, qp, mode, inp, max_range, tud, rows=rows, planes=planes_of(bd, (f - 1) % 3, max_range),
                                    fold_into=None if fold_into is None else fold_into[f - 1]) for f, inp in enumerate(inps, start=1)])


def inputs_of(seed, max_range, pairs, **kw):
    key = ("in", seed, max_range, pairs, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = pu.draw_inputs(seed, max_range, nf=pairs + 1, **kw)
    return _CACHE[key]


def run_plain(torch, ctx, d_luma, origin, stride, fstride, nf, sb, source, recs, tud, qp, max_range, mvp=None, rows=None, stream=None, offsets=(0, 0, 0)):
    """recs [nf - 1, band CTUs, 85] -> the records of the same shape from between canaries; tud None: the entry point without the argument"""
    held, p_in = at_offset(torch, recs, offsets[0])
    mheld, p_mvp = at_offset(torch, mvp, offsets[1]) if mvp is not None else (None, None)
    out = Guarded(torch, recs.size * 16, offsets[2])
    torch.cuda.synchronize()
    p = d_luma.data_ptr() + sb * origin
    if tud is None:
        ctx.motion_rd_device(p, sb, stride, fstride, nf, source, p_in, out.ptr, d_mvp=p_mvp, rows=rows, stream=stream, qp=qp, max_range=max_range)
    else:
        ctx.motion_rd_qt_device(p, sb, stride, fstride, nf, source, p_in, tud, out.ptr, d_mvp=p_mvp, rows=rows, stream=stream, qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    return out.result(RDT, recs.shape)


def run_pu(torch, ctx, d_luma, origin, stride, fstride, nf, sb, mode, dev, shape, tud, qp, max_range, rows=None, stream=None, fold=None, out_offset=0):
    out = Guarded(torch, int(np.prod(shape)) * 16, out_offset)
    torch.cuda.synchronize()
    p, inputs = d_luma.data_ptr() + sb * origin, dev.c if fold is None else dev.with_fold(fold)
    if tud is None:
        ctx.motion_rd_pu_device(p, sb, stride, fstride, nf, mode, inputs, out.ptr, rows=rows, stream=stream, qp=qp, max_range=max_range)
    else:
        ctx.motion_rd_pu_qt_device(p, sb, stride, fstride, nf, mode, inputs, tud, out.ptr, rows=rows, stream=stream, qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    return out.result(RPT, shape)


def records(source, seed, max_range, pairs=1, with_mvp=False):
    return rd.draw_records(source, seed, max_range, shape=(pairs, N, 85), with_mvp=with_mvp)


# ---- 1. the kernel against the restatement: bit depths, plane types, both window layouts, both sources, the depth counts ------------------------------------

CONFIGS = [(np.int16, 8, 8, 22), (np.int16, 10, 33, 37), (np.int16, 12, 64, 27), (np.uint8, 8, 64, 37)]


@pytest.mark.parametrize("dtype,bd,max_range,qp", CONFIGS)
def test_plain_form_equals_the_restatement_and_two_depths_the_existing_entry_point(torch_cuda, dtype, bd, max_range, qp):
    """max_range 8: the MR = 8 layout; 33 and 64: the MR = 64 layout.  Merge records, explicit records against the zero predictor and with predictor records;
    at 3 the restatement, at 2 the bytes of fhevc_motion_rd_device, and the 64x64 and 8x8 nodes equal across the depth counts"""
    torch, sb = torch_cuda, np.dtype(dtype).itemsize
    flat, origin, stride, fstride = plane_batch(bd, 3, dtype)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma = to_dev(torch, flat)
    split2 = 0
    for source, seed, with_mvp in ((rd.MERGE, 5, False), (rd.EXPLICIT, 6, False), (rd.EXPLICIT, 7, True)):
        recs, mvp = records(source, seed, max_range, 2, with_mvp)
        three = run_plain(torch, ctx, d_luma, origin, stride, fstride, 3, sb, source, recs, 3, qp, max_range, mvp=mvp)
        exp = expected_plain(bd, qp, recs, source, max_range, 3, mvp=mvp)
        rd.same(three, exp, (dtype.__name__, bd, max_range, source, with_mvp))
        two = run_plain(torch, ctx, d_luma, origin, stride, fstride, 3, sb, source, recs, 2, qp, max_range, mvp=mvp)
        old = run_plain(torch, ctx, d_luma, origin, stride, fstride, 3, sb, source, recs, None, qp, max_range, mvp=mvp)
        assert two.tobytes() == old.tobytes()
        rd.same(two, expected_plain(bd, qp, recs, source, max_range, 2, mvp=mvp), "two depths")
        assert two[:, :, OUTER].tobytes() == three[:, :, OUTER].tobytes() and (two["cost_rd"] != three["cost_rd"])[:, :, INNER].sum() > 20
        split2 += int(((three["tu_split"] & 0xF0) != 0).sum())
    assert split2 > 30
    ctx.close()


MODE_CONFIGS = [(np.int16, 8, 8, 27), (np.uint8, 8, 64, 22), (np.int16, 10, 33, 37)]


@pytest.mark.parametrize("mode", pu.MODES)
@pytest.mark.parametrize("dtype,bd,max_range,qp", MODE_CONFIGS)
def test_pu_form_equals_the_restatement(torch_cuda, dtype, bd, max_range, qp, mode):
    torch, sb = torch_cuda, np.dtype(dtype).itemsize
    inps = inputs_of(pu.MAIN_SEED, max_range, 2)
    flat, origin, stride, fstride = plane_batch(bd, 3, dtype)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev = to_dev(torch, flat), DevInputs(torch, inps)
    three = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, sb, mode, dev, (2, N, 85), 3, qp, max_range)
    pu.same(three, expected_pu(bd, qp, mode, inps, max_range, 3), (dtype.__name__, bd, max_range, mode))
    two = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, sb, mode, dev, (2, N, 85), 2, qp, max_range)
    old = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, sb, mode, dev, (2, N, 85), None, qp, max_range)
    assert two.tobytes() == old.tobytes() and two[:, :, OUTER].tobytes() == three[:, :, OUTER].tobytes()
    ok = three["part"] != 255
    assert ok.sum() > 80 and (three["cost_rd"][ok] <= rd.SAT).all() and np.array_equal(ok, two["part"] != 255)
    ctx.close()


@pytest.mark.parametrize("with_merge,with_mvp,with_small", [(False, True, True), (True, False, True), (True, True, False)])
def test_pu_form_without_merge_arrays_predictor_records_or_small_pus(torch_cuda, with_merge, with_mvp, with_small):
    torch = torch_cuda
    bd, R, qp = 10, 8, 22
    inps = inputs_of(9, R, 1, with_merge=with_merge, with_mvp=with_mvp, with_small=with_small)
    flat, origin, stride, fstride = plane_batch(bd, 2)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma, dev = to_dev(torch, flat), DevInputs(torch, inps)
    for mode in (0, 1, 6, pu.BEST):
        got = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, 2, mode, dev, (1, N, 85), 3, qp, R)
        pu.same(got, expected_pu(bd, qp, mode, inps, R, 3), (with_merge, with_mvp, with_small, mode))
    ctx.close()


# ---- 2. the fold: a second buffer, in place, across launches of different depth counts ------------------------------------------------------------------------

def test_fold_into_a_second_buffer_in_place_and_across_depth_counts(torch_cuda):
    torch = torch_cuda
    bd, R, qp, pairs = 8, 8, 27, 2
    inps = inputs_of(pu.MAIN_SEED, R, pairs)
    flat, origin, stride, fstride = plane_batch(bd, 3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev = to_dev(torch, flat), DevInputs(torch, inps)
    p_luma, shape = d_luma.data_ptr() + 2 * origin, (pairs, N, 85)
    e0 = expected_pu(bd, qp, 0, inps, R, 3)
    e1 = expected_pu(bd, qp, pu.BEST, inps, R, 3, fold_into=e0)
    e2 = expected_pu(bd, qp, pu.SECOND, inps, R, 3, fold_into=e1)
    first = Guarded(torch, N * 85 * 16 * pairs)
    ctx.motion_rd_pu_qt_device(p_luma, 2, stride, fstride, 3, 0, dev.c, 3, first.ptr, qp=qp, max_range=R)
    torch.cuda.synchronize()
    pu.same(first.result(RPT, shape), e0, "first")
    second = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, 2, pu.BEST, dev, shape, 3, qp, R, fold=first.ptr)
    pu.same(second, e1, "second buffer")
    pu.same(first.result(RPT, shape), e0, "first, after")
    outcomes = np.bincount(pu.fold_outcome(expected_pu(bd, qp, pu.BEST, inps, R, 3), e0).ravel(), minlength=5)
    assert (outcomes[[0, 1, 3, 4]] >= 8).all(), outcomes
    st = torch.cuda.Stream()
    for mode in (pu.BEST, pu.SECOND):
        ctx.motion_rd_pu_qt_device(p_luma, 2, stride, fstride, 3, mode, dev.with_fold(first.ptr), 3, first.ptr, stream=st.cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    pu.same(first.result(RPT, shape), e2, "three launches in place")
    # across depth counts: records of two depths folded into by a launch of three, in place, and the other way round through the old entry point
    m0 = expected_pu(bd, qp, 0, inps, R, 2)
    mixed = Guarded(torch, N * 85 * 16 * pairs)
    ctx.motion_rd_pu_qt_device(p_luma, 2, stride, fstride, 3, 0, dev.c, 2, mixed.ptr, qp=qp, max_range=R)
    ctx.motion_rd_pu_qt_device(p_luma, 2, stride, fstride, 3, pu.BEST, dev.with_fold(mixed.ptr), 3, mixed.ptr, qp=qp, max_range=R)
    torch.cuda.synchronize()
    m1 = expected_pu(bd, qp, pu.BEST, inps, R, 3, fold_into=m0)
    pu.same(mixed.result(RPT, shape), m1, "three folded into two")
    ctx.motion_rd_pu_device(p_luma, 2, stride, fstride, 3, pu.SECOND, dev.with_fold(mixed.ptr), mixed.ptr, qp=qp, max_range=R)
    torch.cuda.synchronize()
    pu.same(mixed.result(RPT, shape), expected_pu(bd, qp, pu.SECOND, inps, R, 2, fold_into=m1), "two folded into the mix")
    ctx.close()


# ---- 3. constructed nodes with values known in advance; a ragged shape --------------------------------------------------------------------------------------

def test_two_constructed_nodes_on_one_pair(torch_cuda):
    """one 64 x 64 pair: a flat reference; the current picture holds, in the 32x32 node 2 (bottom left), a checkerboard inside ONE 8x8 block -- child 3 of its
    depth-1 TU 1 --, and in the 16x16 node at (48, 16) one inside ONE 4x4 block -- child 0 of its depth-1 TU 2.  Known in advance: tu_split = 1 | 1 << (4 + i), a
    cost strictly below the two-depth cost, and every other node of levels 1 and 2 zero (dist 0, bits 2 + side)"""
    torch = torch_cuda
    bd, qp, R = 8, 22, 8
    ref = np.full((64, 64), 128, np.int64)
    cur = ref.copy()
    o32, _ = qt.confined_node(32, 1, 3)
    o16, _ = qt.confined_node(16, 2, 0)
    cur[32:64, 0:32], cur[16:32, 48:64] = o32, o16
    recs = np.zeros((1, 1, 85), MDT)
    recs["cost_best"], recs["idx"] = 10, 1                                   # the zero vector, side bits 2
    k32, k16 = 1 + 2, 5 + 1 * 4 + 3
    assert mr.node_geometry(k32) == (1, 0, 1) and mr.node_geometry(k16) == (2, 3, 1)
    flat, origin, stride, fstride = frames.guarded_plane([ref, cur], bit_depth=bd, dtype=np.int16, poison=5)
    ctx = capi.Context(64, 64, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    got = {t: run_plain(torch, ctx, d_luma, origin, stride, fstride, 2, 2, rd.MERGE, recs, t, qp, R)[0, 0] for t in (2, 3)}
    planes = mr.Planes(ref, bd, 16)
    for t in (2, 3):
        rd.same(got[t][None], qt.expected(cur, ref, 64, 64, bd, qp, recs[0], rd.MERGE, R, t, planes=planes), t)
    lam = rd.lam_q8(qp)
    assert got[3][k32]["tu_split"] == (1 | 1 << 5) and got[3][k16]["tu_split"] == (1 | 1 << 6) and got[2][k32]["tu_split"] == got[2][k16]["tu_split"] == 1
    assert got[3][k32]["cost_rd"] < got[2][k32]["cost_rd"] and got[3][k16]["cost_rd"] < got[2][k16]["cost_rd"]
    for k in range(1, 21):
        if not (cur != ref)[node_rows(k)].any():                            # a node without residual: one cbf bit, one flag bit, the side bits
            assert got[3][k]["dist"] == 0 and got[3][k]["bits"] == 4 and got[3][k]["cost_rd"] == (4 * lam) >> 8 and got[3][k]["tu_split"] == 0, k
    ctx.close()


def test_the_constructed_node_where_the_cbf_condition_of_depth_1_decides(torch_cuda):
    """12 bit, QP 8: the 16x16 node at (16, 32) holds motion_rd_qt_ref.unpaid_node -- its depth-1 TU 1 is coded, dearer than its uncoded children, and must stay
    whole: tu_split = 1 where a kernel without the condition writes 1 | 1 << 5"""
    torch = torch_cuda
    bd, qp, R = qt.UNPAID_BD, qt.UNPAID_QP, 8
    ref = np.full((64, 64), 1 << (bd - 1), np.int64)
    cur = ref.copy()
    cur[32:48, 16:32] = qt.unpaid_node()[0]
    recs = np.zeros((1, 1, 85), MDT)
    recs["cost_best"], recs["idx"] = 10, 1
    k = 5 + 2 * 4 + 1
    assert mr.node_geometry(k) == (2, 1, 2)
    flat, origin, stride, fstride = frames.guarded_plane([ref, cur], bit_depth=bd, dtype=np.int16, poison=5)
    ctx = capi.Context(64, 64, bd, max_frames=2)
    got = run_plain(torch, ctx, to_dev(torch, flat), origin, stride, fstride, 2, 2, rd.MERGE, recs, 3, qp, R)[0, 0]
    rd.same(got[None], qt.expected(cur, ref, 64, 64, bd, qp, recs[0], rd.MERGE, R, 3, planes=mr.Planes(ref, bd, 16)), "unpaid")
    assert got[k]["tu_split"] == 1 and got[k]["bits"] == 64 and got[k]["flags"] == rd.TU_SPLIT
    ctx.close()


def node_rows(k):
    lvl, bx, by = mr.node_geometry(k)
    n = 64 >> lvl
    return (slice(by * n, by * n + n), slice(bx * n, bx * n + n))


def test_a_ragged_72_by_72_picture(torch_cuda):
    torch = torch_cuda
    bd, qp, R = 10, 27, 8
    pics = [p[40:112, 60:132] for p in pictures(bd)[:2]]
    recs, _ = rd.draw_records(rd.MERGE, 12, R, shape=(1, 4, 85))
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=np.int16, poison=9)
    ctx = capi.Context(72, 72, bd, max_frames=2)
    got = run_plain(torch, ctx, to_dev(torch, flat), origin, stride, fstride, 2, 2, rd.MERGE, recs, 3, qp, R)
    exp = qt.expected(pics[1], pics[0], 72, 72, bd, qp, recs[0], rd.MERGE, R, 3)
    rd.same(got[0], exp, "72 x 72")
    valid = exp["cost_rd"] != rd.MARK
    assert valid[0].sum() > 40 and not valid[1:, :21].any() and valid[1:, 21:].any()               # beside the first CTU only 8x8 nodes are whole
    ctx.close()


# ---- 4. bands, poisoned planes, pointers off 16, large batches, streams --------------------------------------------------------------------------------------

def test_bands_are_slices_and_an_empty_band(torch_cuda):
    torch = torch_cuda
    bd, R, qp = 10, 8, 27
    recs, _ = records(rd.MERGE, 31, R, 2)
    inps = inputs_of(31, R, 2)
    flat, origin, stride, fstride = plane_batch(bd, 3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma = to_dev(torch, flat)
    whole = run_plain(torch, ctx, d_luma, origin, stride, fstride, 3, 2, rd.MERGE, recs, 3, qp, R)
    whole_pu = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, 2, pu.BEST, DevInputs(torch, inps), (2, N, 85), 3, qp, R)
    for rows in ((1, 2), (1, 3), (0, 1)):
        sl = slice(rows[0] * CW, rows[1] * CW)
        got = run_plain(torch, ctx, d_luma, origin, stride, fstride, 3, 2, rd.MERGE, np.ascontiguousarray(recs[:, sl]), 3, qp, R, rows=rows)
        assert got.tobytes() == np.ascontiguousarray(whole[:, sl]).tobytes(), rows
        got = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, 2, pu.BEST, DevInputs(torch, [pu.band_of(i, rows) for i in inps]), (2, (rows[1] - rows[0]) * CW, 85), 3,
                     qp, R, rows=rows)
        assert got.tobytes() == np.ascontiguousarray(whole_pu[:, sl]).tobytes(), rows
    out, dev = Guarded(torch, 4096), DevInputs(torch, inps)
    held, p_in = at_offset(torch, recs, 0)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_rd_qt_device(d_luma.data_ptr() + 2 * origin, 2, stride, fstride, 3, rd.MERGE, p_in, 3, out.ptr, rows=(2, 2), qp=qp, max_range=R)
    ctx.motion_rd_pu_qt_device(d_luma.data_ptr() + 2 * origin, 2, stride, fstride, 3, 1, dev.c, 3, out.ptr, rows=(1, 1), qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype,bd,max_range", [(np.int16, 10, 8), (np.uint8, 8, 33), (np.int16, 12, 64)])
def test_guarded_planes_poisoned_margins_odd_origin_and_stride(torch_cuda, dtype, bd, max_range):
    torch, sb = torch_cuda, np.dtype(dtype).itemsize
    flat, origin, stride, fstride = plane_batch(bd, 2, dtype, extra_stride=3, shift=1, frame_gap=5, poison=77)
    assert stride % 2 == 1 and origin % 2 == 1
    recs, _ = records(rd.MERGE, bd + max_range, max_range)
    inps = inputs_of(bd + max_range, max_range, 1)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    got = run_plain(torch, ctx, d_luma, origin, stride, fstride, 2, sb, rd.MERGE, recs, 3, 22, max_range)
    rd.same(got, expected_plain(bd, 22, recs, rd.MERGE, max_range, 3), (dtype.__name__, bd, max_range))
    got = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, sb, 4, DevInputs(torch, inps), (1, N, 85), 3, 22, max_range)
    pu.same(got, expected_pu(bd, 22, 4, inps, max_range, 3), (dtype.__name__, bd, max_range, "pu"))
    ctx.close()


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_pointers_off_their_16_byte_alignment(torch_cuda, offset):
    torch = torch_cuda
    bd, R, qp = 8, 8, 14
    recs, mvp = records(rd.EXPLICIT, 77, R, 1, True)
    inps = inputs_of(77, R, 1)
    flat, origin, stride, fstride = plane_batch(bd, 2)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    aligned = run_plain(torch, ctx, d_luma, origin, stride, fstride, 2, 2, rd.EXPLICIT, recs, 3, qp, R, mvp=mvp)
    rd.same(aligned, expected_plain(bd, qp, recs, rd.EXPLICIT, R, 3, mvp=mvp), "aligned")
    for offsets in ((offset, 0, 0), (0, offset, 0), (0, 0, offset), (offset, 16 - offset, offset)):
        got = run_plain(torch, ctx, d_luma, origin, stride, fstride, 2, 2, rd.EXPLICIT, recs, 3, qp, R, mvp=mvp, offsets=offsets)
        assert got.tobytes() == aligned.tobytes(), offsets
    base = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, 2, pu.BEST, DevInputs(torch, inps), (1, N, 85), 3, qp, R)
    pu.same(base, expected_pu(bd, qp, pu.BEST, inps, R, 3), "pu aligned")
    got = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, 2, pu.BEST, DevInputs(torch, inps, offset), (1, N, 85), 3, qp, R, out_offset=offset)
    assert got.tobytes() == base.tobytes()
    held, p_fold = at_offset(torch, base, offset)
    again = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, 2, pu.SECOND, DevInputs(torch, inps), (1, N, 85), 3, qp, R, fold=p_fold, out_offset=16 - offset)
    pu.same(again, expected_pu(bd, qp, pu.SECOND, inps, R, 3, fold_into=base), "fold off 16")
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_more_ctus_than_the_persistent_grid(torch_cuda, max_range):
    """116 picture pairs of 9 CTUs = 1 044 CTUs in one launch: two pictures alternate and the records repeat, so pair f equals pair f - 2; the first two pairs
    equal the restatement"""
    torch = torch_cuda
    a, b = pictures(8)[:2]
    NF = 117
    assert (NF - 1) * N > 4 * 256
    two, _ = records(rd.MERGE, max_range, max_range, 2)
    ctx = capi.Context(W, H, 8, max_frames=NF)
    flat = np.stack([a, b] * (NF // 2) + [a]).astype(np.uint8)
    got = run_plain(torch, ctx, to_dev(torch, flat), 0, W, W * H, NF, 1, rd.MERGE, np.concatenate([two] * (NF // 2)), 3, 22, max_range)
    exp = np.stack([qt.expected(b, a, W, H, 8, 22, two[0], rd.MERGE, max_range, 3, planes=planes_of(8, 0, max_range)),
                    qt.expected(a, b, W, H, 8, 22, two[1], rd.MERGE, max_range, 3, planes=planes_of(8, 1, max_range))])
    rd.same(got[:2], exp, "first pairs")
    first = got[:2].tobytes()
    for f in range(2, NF - 1, 2):
        assert got[f:f + 2].tobytes() == first, f
    ctx.close()


def test_two_streams_with_different_qps_ranges_and_depth_counts(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, origin, stride, fstride = plane_batch(bd, 3)
    calls = [(10, 8, 3), (51, 64, 2), (27, 8, 2), (22, 33, 3), (37, 64, 3), (14, 8, 3)]
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    recs = [records(rd.MERGE, 100 + i, R, 2)[0] for i, (_, R, _) in enumerate(calls)]
    held = [at_offset(torch, r, 0) for r in recs]
    outs = [Guarded(torch, 2 * N * 85 * 16) for _ in calls]
    torch.cuda.synchronize()
    for i, (qp, R, tud) in enumerate(calls):
        ctx.motion_rd_qt_device(d_luma.data_ptr() + 2 * origin, 2, stride, fstride, 3, rd.MERGE, held[i][1], tud, outs[i].ptr, stream=streams[i % 2].cuda_stream, qp=qp,
                                max_range=R)
    torch.cuda.synchronize()
    for i, (qp, R, tud) in enumerate(calls):
        rd.same(outs[i].result(RDT, (2, N, 85)), expected_plain(bd, qp, recs[i], rd.MERGE, R, tud), i)
    ctx.close()


# ---- 5. the chain on one stream, the intra stage on its records, the frame call --------------------------------------------------------------------------------

def device_chain(torch, ctx, p, sb, stride, fstride, qp, R, coarse, skip_mask, tud, stream):
    """search -> refinement -> re-pricing -> merge stages -> selection -> the four RD launches at tud -> the RD tree, through the device forms on one stream
    without a host synchronisation -> dict of Guarded outputs"""
    g = {k: Guarded(torch, N * per * 16) for k, per in (("found", 85), ("found_pu", 124), ("found_s", 384), ("fine", 85), ("fine_pu", 124), ("fine_s", 384),
                                                          ("priced", 85), ("priced_pu", 124), ("priced_s", 384), ("merge", 85), ("merge_pu", 124), ("merge_s", 384),
                                                          ("shapes", 85), ("rd_merge", 85), ("rd_pu", 85), ("centres", 1))}
    g.update({k: Guarded(torch, N * per * 8) for k, per in (("mvp", 85), ("mvp_pu", 124), ("mvp_s", 384))})
    g.update(dmin=Guarded(torch, N * 256), dmax=Guarded(torch, N * 256))
    torch.cuda.synchronize()
    s = stream.cuda_stream
    if coarse:
        ctx.motion_centres_device(p, sb, stride, fstride, 2, g["centres"].ptr, stream=s, qp=qp, coarse_range=coarse)
        ctx.motion_search_pu_centred_device(p, sb, stride, fstride, 2, g["centres"].ptr, g["found"].ptr, g["found_pu"].ptr, g["found_s"].ptr, stream=s, qp=qp, search_range=R)
        ctx.motion_refine_pu_centred_device(p, sb, stride, fstride, 2, g["centres"].ptr, g["found"].ptr, g["fine"].ptr, g["found_pu"].ptr, g["fine_pu"].ptr,
                                            g["found_s"].ptr, g["fine_s"].ptr, stream=s, qp=qp, max_range=R)
    else:
        ctx.motion_search_pu_wide_device(p, sb, stride, fstride, 2, g["found"].ptr, g["found_pu"].ptr, g["found_s"].ptr, stream=s, qp=qp, search_range=R)
        ctx.motion_refine_pu_wide_device(p, sb, stride, fstride, 2, g["found"].ptr, g["fine"].ptr, g["found_pu"].ptr, g["fine_pu"].ptr, g["found_s"].ptr, g["fine_s"].ptr,
                                         stream=s, qp=qp, max_range=R)
    ctx.motion_amvp_device(2, g["fine"].ptr, g["fine_pu"].ptr, g["fine_s"].ptr, g["priced"].ptr, g["priced_pu"].ptr, g["priced_s"].ptr, g["mvp"].ptr, g["mvp_pu"].ptr,
                           g["mvp_s"].ptr, stream=s, qp=qp)
    Rm = 64 if coarse else R
    ctx.motion_merge_device(p, sb, stride, fstride, 2, g["priced"].ptr, g["merge"].ptr, stream=s, qp=qp, max_range=Rm)
    ctx.motion_merge_pu_device(p, sb, stride, fstride, 2, g["priced"].ptr, g["merge_pu"].ptr, g["merge_s"].ptr, stream=s, qp=qp, max_range=Rm)
    ctx.pu_shape_select_merge_device(g["priced"].ptr, g["priced_pu"].ptr, g["priced_s"].ptr, g["merge_pu"].ptr, g["merge_s"].ptr, 1, g["shapes"].ptr, stream=s)
    ctx.motion_rd_qt_device(p, sb, stride, fstride, 2, rd.MERGE, g["merge"].ptr, tud, g["rd_merge"].ptr, stream=s, qp=qp, max_range=Rm)
    inputs = ctx.rd_pu_inputs(g["priced"].ptr, g["priced_pu"].ptr, g["priced_s"].ptr, g["merge_pu"].ptr, g["merge_s"].ptr, g["mvp"].ptr, g["mvp_pu"].ptr, g["mvp_s"].ptr,
                              g["shapes"].ptr)
    ctx.motion_rd_pu_qt_device(p, sb, stride, fstride, 2, 0, inputs, tud, g["rd_pu"].ptr, stream=s, qp=qp, max_range=Rm)
    inputs.fold = g["rd_pu"].ptr
    for mode in (pu.BEST, pu.SECOND):
        ctx.motion_rd_pu_qt_device(p, sb, stride, fstride, 2, mode, inputs, tud, g["rd_pu"].ptr, stream=s, qp=qp, max_range=Rm)
    ctx.p_tree_select_rd_pu_device(g["rd_pu"].ptr, g["rd_merge"].ptr, skip_mask, 1, g["dmin"].ptr, g["dmax"].ptr, stream=s)
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("coarse", [0, 6])
def test_the_chain_on_one_stream_and_the_frame_call(torch_cuda, coarse):
    """every RD output of the chain at three depths against the restatement on the device's own intermediate records; fhevc_p_tree_rd_qt_frame against those
    pieces, with what it moves and launches; at 2 against fhevc_p_tree_rd_frame"""
    torch = torch_cuda
    bd, R, qp, mask = 8, 8, 27, 3
    ys = frames.pan_clip(W, H, 2, seed=39, v_structure=-5, v_noise=3)
    pics = [y.astype(np.int64) for y in ys]
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=np.uint8, poison=None)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    ctx.enable_kernel_timing(True)
    for s in (29, 31, 35):
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    g = device_chain(torch, ctx, d_luma.data_ptr() + origin, 1, stride, fstride, qp, R, coarse, mask, 3, torch.cuda.Stream())
    launched = ctx.stats()["kernels_launched"] - launched
    assert ctx.kernel_timing(35)[1] == 4 and ctx.kernel_timing(29)[1] == 0 and ctx.kernel_timing(31)[1] == 0
    ctx.enable_kernel_timing(False)
    Rm = 64 if coarse else R
    inp = pu.Inputs(g["priced"].result(QDT, (N, 85)), g["priced_pu"].result(QDT, (N, 124)), g["priced_s"].result(QDT, (N, 384)), g["merge_pu"].result(MDT, (N, 124)),
                    g["merge_s"].result(MDT, (N, 384)), g["mvp"].result(PDT, (N, 85)), g["mvp_pu"].result(PDT, (N, 124)), g["mvp_s"].result(PDT, (N, 384)),
                    g["shapes"].result(SDT, (N, 85)))
    merge = g["merge"].result(MDT, (N, 85))
    e_merge, e_pu, emin, emax = qt.frame_records(pics[1], pics[0], W, H, bd, qp, Rm, inp, merge, mask, 3, planes=mr.Planes(pics[0], bd, 16 if Rm <= 8 else 72))
    got_pu = g["rd_pu"].result(RPT, (N, 85))
    rd.same(g["rd_merge"].result(RDT, (N, 85)), e_merge, "rd of the merge records")
    pu.same(got_pu, e_pu, "folded")
    assert np.array_equal(g["dmin"].result(np.uint8, (N, 256)), emin) and np.array_equal(g["dmax"].result(np.uint8, (N, 256)), emax)
    assert (got_pu["part"] != 255).sum() > 300
    # the frame call: the same bytes from host buffers
    planes = [pel(p) for p in pics]
    kw = dict(origin=planes[0][1], stride=planes[0][2], qp=qp, search_range=R, coarse_range=coarse, skip_mask=mask)
    before = ctx.stats()
    out = ctx.p_tree_rd_qt_frame(planes[1][0], planes[0][0], 3, with_shapes=True, with_merge=True, with_rd_merge=True, with_rd_pu=True, **kw)
    after = ctx.stats()
    for name, a, dt, per in zip(("dmin", "dmax", "shapes", "merge", "rd_merge", "rd_pu"), out, (np.uint8, np.uint8, SDT, MDT, RDT, RPT), (256, 256, 85, 85, 85, 85)):
        assert a.tobytes() == g[name].result(dt, (N, per)).tobytes(), name
    assert after["bytes_h2d"] - before["bytes_h2d"] == 4 * W * H and after["bytes_d2h"] - before["bytes_d2h"] == N * (2 * 256 + 4 * 85 * 16)
    assert after["kernels_launched"] - before["kernels_launched"] == launched >= 13
    # at two depths: fhevc_p_tree_rd_frame's bytes
    two = ctx.p_tree_rd_qt_frame(planes[1][0], planes[0][0], 2, with_rd_merge=True, with_rd_pu=True, **kw)
    old = ctx.p_tree_rd_frame(planes[1][0], planes[0][0], with_rd_merge=True, with_rd_pu=True, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(two, old)) and two[3].tobytes() != out[5].tobytes()
    ctx.close()


def test_the_folded_records_as_d_fold_of_the_intra_stage(torch_cuda):
    """records folded at three depths go into fhevc_intra_rd_device unchanged, in place: the restatement of the intra stage on the restated records"""
    torch = torch_cuda
    bd, R, qp = 8, 8, 27
    inp = inputs_of(pu.MAIN_SEED, R, 1)[0]
    recs, _ = records(rd.MERGE, 5, R)
    flat, origin, stride, fstride = plane_batch(bd, 2)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    p = d_luma.data_ptr() + 2 * origin
    cur = pictures(bd)[1]
    first = ir.draw_first(cur, bd, qp, 3, False)
    folded = expected_pu(bd, qp, 0, [inp], R, 3)[0]
    rd_merge = expected_plain(bd, qp, recs, rd.MERGE, R, 3)[0]
    exp = ir.expected(cur, bd, qp, first, fold=folded, rd_merge=rd_merge, skip_mask=3)
    dev, out, d_merge = DevInputs(torch, [inp]), Guarded(torch, N * 85 * 16), Guarded(torch, N * 85 * 16)
    h_first, p_first = at_offset(torch, first, 0)
    h_recs, p_recs = at_offset(torch, recs, 0)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.motion_rd_qt_device(p, 2, stride, fstride, 2, rd.MERGE, p_recs, 3, d_merge.ptr, stream=st.cuda_stream, qp=qp, max_range=R)
    ctx.motion_rd_pu_qt_device(p, 2, stride, fstride, 2, 0, dev.c, 3, out.ptr, stream=st.cuda_stream, qp=qp, max_range=R)
    ctx.intra_rd_device(p + 2 * fstride, 2, stride, 0, 1, p_first, out.ptr, d_fold=out.ptr, d_rd_merge=d_merge.ptr, skip_mask=3, stream=st.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    got = out.result(RPT, (N, 85))
    ir.same(got, exp, "intra folded into three depths")
    assert (got["part"] == capi.RD_PART_INTRA).sum() > 8 and (got["part"] == 0).sum() > 8 and ((got["tu_split"] & 0xF0) != 0).sum() > 8
    ctx.close()


@pytest.mark.parametrize("max_range,mode,fold", [(8, 1, False), (64, pu.BEST, True)])
def test_host_forms_equal_device_forms_and_count_what_they_move(torch_cuda, max_range, mode, fold):
    torch = torch_cuda
    bd, qp = 10, 22
    inp = inputs_of(3, max_range, 1)[0]
    recs, mvp = records(rd.EXPLICIT, 3, max_range, 1, True)
    flat, origin, stride, fstride = plane_batch(bd, 2)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    planes = [pel(p) for p in pictures(bd)[:2]]
    kw = dict(origin=planes[0][1], stride=planes[0][2], qp=qp, max_range=max_range)
    dev = run_plain(torch, ctx, d_luma, origin, stride, fstride, 2, 2, rd.EXPLICIT, recs, 3, qp, max_range, mvp=mvp)
    before = ctx.stats()
    host = ctx.motion_rd_qt(planes[1][0], planes[0][0], recs[0], rd.EXPLICIT, 3, mvp=mvp[0], **kw)
    after = ctx.stats()
    assert host.tobytes() == dev[0].tobytes() and (host["cost_rd"] != rd.MARK).sum() > 100
    assert after["bytes_h2d"] - before["bytes_h2d"] == 4 * W * H + N * 85 * 24 and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    earlier = expected_pu(bd, qp, 0, [inp], max_range, 2)[0] if fold else None
    held, p_fold = at_offset(torch, earlier, 0) if fold else (None, None)
    dev = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, 2, mode, DevInputs(torch, [inp]), (1, N, 85), 3, qp, max_range, fold=p_fold)
    before = ctx.stats()
    host = ctx.motion_rd_pu_qt(planes[1][0], planes[0][0], mode, inp.nodes, 3, *inp[1:], fold=earlier, **kw)
    after = ctx.stats()
    assert host.tobytes() == dev[0].tobytes() and (host["part"] != 255).sum() > 100
    moved = N * (16 * (85 + 124 + 384) + 16 * (124 + 384) + 8 * (85 + 124 + 384) + 16 * 85 + (16 * 85 if fold else 0))
    assert after["bytes_h2d"] - before["bytes_h2d"] == 4 * W * H + moved and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    for tud in (1, 4):
        with pytest.raises(capi.FastHevcError):
            ctx.motion_rd_qt(planes[1][0], planes[0][0], recs[0], rd.EXPLICIT, tud, mvp=mvp[0], **kw)
        with pytest.raises(capi.FastHevcError):
            ctx.motion_rd_pu_qt(planes[1][0], planes[0][0], mode, inp.nodes, tud, *inp[1:], **kw)
    assert ctx.stats() == after
    ctx.close()


# ---- 6. rejected calls, the timing slot ----------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, origin, stride, fstride = plane_batch(bd, 3)
    inps = inputs_of(8, 8, 2)
    recs, mvp = records(rd.EXPLICIT, 8, 8, 2, True)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev = to_dev(torch, flat), DevInputs(torch, inps)
    h_in, p_in = at_offset(torch, recs, 0)
    h_mvp, p_mvp = at_offset(torch, mvp, 0)
    out = Guarded(torch, 2 * N * 85 * 16 + 64)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr() + 2 * origin, sb=2, stride=stride, fs=fstride, nf=3, rb=0, re=CH, qp=30, R=8, tud=3, out=out.ptr)
    common = [(dict(ctx=None), None), (dict(luma=None), "argument"), (dict(out=None), "argument"), (dict(nf=1), "layout"), (dict(sb=3), "layout"),
              (dict(stride=W - 1), "layout"), (dict(qp=52), "qp"), (dict(R=0), "max_range"), (dict(R=65), "max_range"), (dict(rb=2, re=1), "band"),
              (dict(re=CH + 1), "band"), (dict(out=out.ptr + 2), "aligned"), (dict(tud=1), "tu_depths"), (dict(tud=4), "tu_depths"), (dict(tud=0), "tu_depths"),
              (dict(tud=-3), "tu_depths")]
    launched = ctx.stats()["kernels_launched"]

    def plain(a):
        return lib.fhevc_motion_rd_qt_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a.get("source", 1),
                                             a.get("in_", p_in), a.get("mvp", p_mvp), a["tud"], a["out"], None)

    def with_pu(a):
        inputs = capi.MotionRdPuInputs(**a.get("inputs", dev.ptrs))
        return lib.fhevc_motion_rd_pu_qt_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a.get("mode", 8),
                                                C.byref(inputs), a["tud"], a["out"], None)
    for call, more in ((plain, [(dict(source=2), "source"), (dict(source=0), "explicit"), (dict(in_=None), "argument"), (dict(mvp=p_mvp + 2), "aligned")]),
                       (with_pu, [(dict(mode=3), "part_mode"), (dict(mode=10), "part_mode"), (dict(inputs=dict(dev.ptrs, shapes=None)), "selection"),
                                  (dict(inputs=dict(dev.ptrs, fold=out.ptr + 16)), "overlaps")])):
        for change, text in common + more:
            assert call(dict(good, **change)) == capi.E_INVALID, change
            if text:
                assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    # the frame call
    planes = [pel(p) for p in pictures(bd)[:2]]
    maps = np.full(2 * N * 256, CANARY, np.uint8)
    for kw in (dict(tud=1), dict(tud=4), dict(qp=52), dict(skip_mask=4), dict(search_range=65), dict(coarse_range=15)):
        a = dict(dict(qp=30, search_range=8, coarse_range=0, skip_mask=3, tud=3), **kw)
        rc = lib.fhevc_p_tree_rd_qt_frame(ctx.h, planes[1][0].ctypes.data + 2 * planes[0][1], planes[0][0].ctypes.data + 2 * planes[0][1], planes[0][2], a["qp"],
                                          a["search_range"], a["coarse_range"], None, None, a["skip_mask"], a["tud"], maps.ctypes.data, maps.ctypes.data + N * 256, None,
                                          None, None, None)
        assert rc == capi.E_INVALID and (maps == CANARY).all(), kw
    assert ctx.stats()["kernels_launched"] == launched
    assert plain(good) == capi.OK and with_pu(good) == capi.OK            # the same calls with nothing wrong are accepted
    torch.cuda.synchronize()
    assert not out.untouched()
    ctx.close()


def test_slot_35_counts_one_launch_per_call_and_the_other_slots_stay_untouched(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, origin, stride, fstride = plane_batch(bd, 3)
    recs, _ = records(rd.MERGE, 8, 8, 2)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev, out = to_dev(torch, flat), DevInputs(torch, inputs_of(8, 8, 2)), Guarded(torch, 2 * N * 85 * 16)
    held, p_in = at_offset(torch, recs, 0)
    p = d_luma.data_ptr() + 2 * origin
    torch.cuda.synchronize()
    ctx.enable_kernel_timing(True)
    slots = (17, 29, 31, 33, 35)
    for s in slots:
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    calls = 0
    for R, mode in ((8, None), (64, 8), (8, 5), (64, None)):
        if mode is None:
            ctx.motion_rd_qt_device(p, 2, stride, fstride, 3, rd.MERGE, p_in, 3, out.ptr, qp=30, max_range=R)
        else:
            ctx.motion_rd_pu_qt_device(p, 2, stride, fstride, 3, mode, dev.c, 3, out.ptr, qp=30, max_range=R)
        torch.cuda.synchronize()
        calls += 1
        ms, count = ctx.kernel_timing(35)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (17, 29, 31, 33))
    # two depths count under the mirrored calls' slots
    ctx.motion_rd_qt_device(p, 2, stride, fstride, 3, rd.MERGE, p_in, 2, out.ptr, qp=30, max_range=8)
    ctx.motion_rd_pu_qt_device(p, 2, stride, fstride, 3, 0, dev.c, 2, out.ptr, qp=30, max_range=8)
    torch.cuda.synchronize()
    assert [ctx.kernel_timing(s)[1] for s in slots] == [0, 1, 1, 0, 4]
    ctx.enable_kernel_timing(False)
    for s in (34, 36):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()
