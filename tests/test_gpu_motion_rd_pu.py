"""Config 4 (P slices): the RD stage under a partition size (the PU instances of k_motion_rd.hip), its fold, the RD tree on folded records and the frame
call that chains them, on the MI355X, byte for byte against the Python restatement tests/motion_rd_pu_ref.py (which tests/test_motion_rd_pu_ref.py
checks without a GPU, together with what the draw below holds).  Nothing is compared with the kernel's own output except where two launches must give
the same bytes, and where the stage must agree with an existing kernel: 2Nx2N with fhevc_motion_rd_device, `merged` with the selection's bits.

Pictures are the RD tests' draw, 168 x 152 = 3 x 3 CTUs, ragged in both directions; the main draw is six picture pairs over its three pictures."""
import ctypes as C

import numpy as np
import pytest

import motion_rd_pu_ref as pu
import motion_rd_ref as rd
import motion_refine_ref as mr
import p_tree_ref as tr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)
from test_gpu_motion_rd import Guarded, at_offset, pictures, planes_of

pytestmark = pytest.mark.gpu

W, H, CW, CH, N = pu.W, pu.H, pu.CW, pu.CH, pu.N
QDT, MDT, PDT, SDT, RDT, RPT, TDT = (capi.MOTION_QPEL_DTYPE, capi.MOTION_MERGE_DTYPE, capi.MOTION_MVP_DTYPE, capi.SHAPE_DTYPE, capi.MOTION_RD_DTYPE,
                                     capi.MOTION_RD_PU_DTYPE, capi.TREE_DTYPE)
_CACHE = {}


def frames_of(bd, nf):
    """nf frames over the draw's three pictures: frame f is predicted from frame f - 1"""
    return [pictures(bd)[f % 3] for f in range(nf)]


def inputs_of(seed, max_range, pairs, **kw):
    key = ("in", seed, max_range, pairs, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = pu.draw_inputs(seed, max_range, nf=pairs + 1, **kw)
    return _CACHE[key]


def expected_batch(bd, qp, mode, inps, max_range, rows=None, fold_into=None):
    """inps: one Inputs per picture pair -> [pairs, band CTUs, 85]"""
    out = []
    for f, inp in enumerate(inps, start=1):
        pics = pictures(bd)
        out.append(pu.expected(pics[f % 3], pics[(f - 1) % 3], W, H, bd, qp, mode, inp, max_range, rows=rows, planes=planes_of(bd, (f - 1) % 3, max_range),
                               fold_into=None if fold_into is None else fold_into[f - 1]))
    return np.stack(out)


class DevInputs:
    """the arrays of a list of Inputs (one per picture pair) on the device, each `offset` bytes behind a 16-byte boundary, as a MotionRdPuInputs"""

    def __init__(self, torch, inps, offset=0, only=None):
        self.held, ptrs = [], {}
        for name in pu.Inputs._fields:
            arrays = [getattr(i, name) for i in inps]
            if arrays[0] is None:
                continue
            t, p = at_offset(torch, np.stack(arrays), offset if only in (None, name) else 0)
            self.held.append(t)
            ptrs[name] = p
        self.ptrs = ptrs
        self.c = capi.MotionRdPuInputs(**ptrs)

    def with_fold(self, ptr):
        return capi.MotionRdPuInputs(fold=ptr, **self.ptrs)


def plane_batch(bd, nf, dtype=np.int16, **kw):
    return frames.guarded_plane(frames_of(bd, nf), bit_depth=bd, dtype=dtype, poison=kw.pop("poison", None), **kw)


def run_pu(torch, ctx, d_luma, origin, stride, fstride, nf, sb, mode, dev, shape, qp, max_range, rows=None, stream=None, fold=None, out_offset=0):
    """one launch -> [pairs, band CTUs, 85] records from between canaries; fold: None, or the device address of earlier records"""
    out = Guarded(torch, int(np.prod(shape)) * 16, out_offset)
    torch.cuda.synchronize()
    ctx.motion_rd_pu_device(d_luma.data_ptr() + sb * origin, sb, stride, fstride, nf, mode, dev.c if fold is None else dev.with_fold(fold), out.ptr, rows=rows,
                            stream=stream, qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    return out.result(RPT, shape)


# ---- 1. the kernel against the restatement: every size, bit depths, plane types, both window layouts ----------------------------------------------------

CONFIGS = [(np.int16, 8, 8, 27, pu.MAIN_PAIRS), (np.int16, 10, 33, 37, 2), (np.int16, 12, 64, 22, 2), (np.uint8, 8, 64, 10, 2)]


@pytest.mark.parametrize("mode", pu.MODES)
@pytest.mark.parametrize("dtype,bd,max_range,qp,pairs", CONFIGS)
def test_kernel_equals_the_restatement(torch_cuda, dtype, bd, max_range, qp, pairs, mode):
    """max_range 8: the MR = 8 layout; 33 and 64: the MR = 64 layout with a part of its window and with the whole of it staged"""
    sb, nf = np.dtype(dtype).itemsize, pairs + 1
    inps = inputs_of(pu.MAIN_SEED, max_range, pairs)
    flat, origin, stride, fstride = plane_batch(bd, nf, dtype)
    ctx = capi.Context(W, H, bd, max_frames=nf)
    got = run_pu(torch_cuda, ctx, to_dev(torch_cuda, flat), origin, stride, fstride, nf, sb, mode, DevInputs(torch_cuda, inps), (pairs, N, 85), qp, max_range)
    pu.same(got, expected_batch(bd, qp, mode, inps, max_range), (dtype.__name__, bd, max_range, mode))
    ok = got["part"] != 255
    assert ok.sum() > 40 * pairs and (got["cost_rd"][ok] <= rd.SAT).all() and (got["cost_rd"][~ok] == rd.MARK).all()
    if mode in pu.TWO_PART:
        assert (got["part"][ok] == mode).all() and set(np.unique(got["merged"][ok])) == {0, 1, 2, 3}
    ctx.close()


@pytest.mark.parametrize("with_merge,with_mvp,with_small", [(False, True, True), (True, False, True), (False, False, True), (True, True, False)])
def test_without_merge_arrays_predictor_records_or_small_pus(torch_cuda, with_merge, with_mvp, with_small):
    bd, R, qp, pairs = 10, 8, 22, 1
    inps = inputs_of(9, R, pairs, with_merge=with_merge, with_mvp=with_mvp, with_small=with_small)
    flat, origin, stride, fstride = plane_batch(bd, 2)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma, dev = to_dev(torch_cuda, flat), DevInputs(torch_cuda, inps)
    for mode in (0, 1, 6, pu.BEST, pu.SECOND):
        got = run_pu(torch_cuda, ctx, d_luma, origin, stride, fstride, 2, 2, mode, dev, (pairs, N, 85), qp, R)
        pu.same(got, expected_batch(bd, qp, mode, inps, R), (with_merge, with_mvp, with_small, mode))
        if not with_merge:
            assert not got["merged"].any()
        if not with_small and mode == 6:
            lvl2 = got[:, :, 5:21]
            assert (lvl2["part"] == 255).all() and (got[:, :, 21:]["part"] == 255).all()          # AMP of the 16x16 nodes lives in the small family
    ctx.close()


# ---- 2. against the existing kernels ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_mvp", [False, True])
def test_2Nx2N_equals_the_rd_stage_on_bytes_0_to_11(torch_cuda, with_mvp):
    torch = torch_cuda
    bd, R, qp = 10, 33, 27
    inps = inputs_of(21, R, 2, with_mvp=with_mvp)
    flat, origin, stride, fstride = plane_batch(bd, 3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev = to_dev(torch, flat), DevInputs(torch, inps)
    got = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, 2, 0, dev, (2, N, 85), qp, R)
    base = Guarded(torch, 2 * N * 85 * 16)
    ctx.motion_rd_device(d_luma.data_ptr() + 2 * origin, 2, stride, fstride, 3, rd.EXPLICIT, dev.ptrs["nodes"], base.ptr, d_mvp=dev.ptrs.get("mvp_nodes"), qp=qp, max_range=R)
    torch.cuda.synchronize()
    b = base.result(RDT, (2, N, 85))
    assert np.array_equal(got.view(np.uint8).reshape(-1, 16)[:, :12], b.view(np.uint8).reshape(-1, 16)[:, :12])
    ok = b["cost_rd"] != rd.MARK
    assert ok.sum() > 400 and (got["part"][ok] == 0).all() and (got["part"][~ok] == 255).all() and not got["merged"].any() and not got["pad"].any()
    ctx.close()


def test_merged_equals_the_selections_bits_for_the_size_priced(torch_cuda):
    torch = torch_cuda
    bd, R, qp = 8, 8, 27
    inps = inputs_of(pu.MAIN_SEED, R, 2)
    flat, origin, stride, fstride = plane_batch(bd, 3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev = to_dev(torch, flat), DevInputs(torch, inps)
    shapes, merged = Guarded(torch, 2 * N * 85 * 16), Guarded(torch, 2 * N * 85 * 2)
    ctx.pu_shape_select_merge_device(dev.ptrs["nodes"], dev.ptrs["pus"], dev.ptrs["pus_small"], dev.ptrs["merge_pus"], dev.ptrs["merge_pus_small"], 2, shapes.ptr,
                                     d_merged=merged.ptr)
    torch.cuda.synchronize()
    bits = merged.result(np.uint16, (2, N, 85)).astype(np.int64)
    seen = 0
    for p in pu.TWO_PART:
        got = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, 2, p, dev, (2, N, 85), qp, R)
        ok = got["part"] == p
        assert np.array_equal(got["merged"][ok], ((bits >> (2 * p)) & 3)[ok]), p
        seen += int(ok.sum())
    assert seen > 1500
    ctx.close()


# ---- 3. pictures built by the filter itself: straddling tiles decide the result ---------------------------------------------------------------------------

QA, QB = (5, 2), (-6, 7)


@pytest.mark.parametrize("bd,max_range,qp", [(8, 8, 27), (10, 33, 37)])
def test_constructed_pictures_through_the_kernel(torch_cuda, bd, max_range, qp):
    """ten CTUs, one per kind: with the true vectors in the parts that size has dist 0 and the closed-form bits and cost; the node forced to 2Nx2N at either
    vector has dist > 0; the fold of the two keeps the two-part size, whichever comes first"""
    torch = torch_cuda
    n = len(pu.KIND_ORDER)
    rng = np.random.default_rng(3 + bd)
    yy, xx = np.mgrid[0:64, 0:64 * n].astype(np.float64)
    top = (1 << bd) - 1
    ref = np.clip((0.5 + 0.2 * np.sin(xx / 7.0) * np.cos(yy / 5.0)) * top + rng.normal(0, 0.08 * top, size=xx.shape), 0, top).astype(np.int64)
    planes = mr.Planes(ref, bd, 16 if max_range <= 8 else 72)
    cur = pu.two_motion_picture(planes, pu.KIND_ORDER, QA, QB)
    inp = pu.two_motion_inputs(pu.KIND_ORDER, QA, QB)
    at_b = inp._replace(nodes=pu.two_motion_inputs(pu.KIND_ORDER, QB, QA).nodes)
    flat, origin, stride, fstride = frames.guarded_plane([ref, cur], bit_depth=bd, dtype=np.int16, poison=5)
    ctx = capi.Context(64 * n, 64, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    lam = rd.lam_q8(qp)
    side = sum(mr.eg_bits(v) for v in QA + QB)

    def launch(x, mode, fold=None):
        out = Guarded(torch, n * 85 * 16)
        dev = DevInputs(torch, [x])
        if fold is not None:
            out.t[out.off:out.off + out.n] = torch.from_numpy(fold.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        ctx.motion_rd_pu_device(d_luma.data_ptr() + 2 * origin, 2, stride, fstride, 2, mode, dev.c if fold is None else dev.with_fold(out.ptr), out.ptr, qp=qp,
                                max_range=max_range)
        torch.cuda.synchronize()
        return out.result(RPT, (n, 85))

    whole = [launch(x, 0) for x in (inp, at_b)]
    for x, w in zip((inp, at_b), whole):
        pu.same(w, pu.expected(cur, ref, 64 * n, 64, bd, qp, 0, x, max_range, planes=planes), "2Nx2N")
    for i, kind in enumerate(pu.KIND_ORDER):
        p = pu.part_size_of_kind(kind)
        two = launch(inp, p)
        pu.same(two, pu.expected(cur, ref, 64 * n, 64, bd, qp, p, inp, max_range, planes=planes), kind)
        folded = [launch(inp, p, fold=w) for w in whole] + [launch(x, 0, fold=two) for x in (inp, at_b)]     # in place, either order
        for k in pu.TWO_MOTION_KINDS[kind][2]:
            r = two[i, k]
            assert r["dist"] == 0 and r["flags"] & 1 and r["part"] == p and r["bits"] == side + 2 * (4 if k == 0 else 1), (kind, k, r)
            assert r["cost_rd"] == (lam * int(r["bits"])) >> 8 and whole[0][i, k]["dist"] > 0 and whole[1][i, k]["dist"] > 0, (kind, k, r)
            assert all(f[i, k].tobytes() == r.tobytes() for f in folded), (kind, k)
    ctx.close()


# ---- 4. the fold -----------------------------------------------------------------------------------------------------------------------------------------

def test_fold_into_a_second_buffer_in_place_with_itself_and_the_three_launches(torch_cuda):
    torch = torch_cuda
    bd, R, qp, pairs = 8, 8, 27, 2
    inps = inputs_of(pu.MAIN_SEED, R, pairs)
    flat, origin, stride, fstride = plane_batch(bd, 3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev = to_dev(torch, flat), DevInputs(torch, inps)
    p_luma = d_luma.data_ptr() + 2 * origin
    shape = (pairs, N, 85)
    e0 = expected_batch(bd, qp, 0, inps, R)
    e1 = expected_batch(bd, qp, pu.BEST, inps, R, fold_into=e0)
    e2 = expected_batch(bd, qp, pu.SECOND, inps, R, fold_into=e1)
    first = Guarded(torch, N * 85 * 16 * pairs)
    ctx.motion_rd_pu_device(p_luma, 2, stride, fstride, 3, 0, dev.c, first.ptr, qp=qp, max_range=R)
    torch.cuda.synchronize()
    pu.same(first.result(RPT, shape), e0, "first")
    # into a second buffer: the earlier records stay what they were
    second = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, 2, pu.BEST, dev, shape, qp, R, fold=first.ptr)
    pu.same(second, e1, "second buffer")
    pu.same(first.result(RPT, shape), e0, "first, after")
    outcomes = np.bincount(pu.fold_outcome(expected_batch(bd, qp, pu.BEST, inps, R), e0).ravel(), minlength=5)
    assert (outcomes[[0, 1, 3, 4]] >= 8).all(), outcomes
    # in place, the three-launch sequence on one stream
    st = torch.cuda.Stream()
    for mode in (pu.BEST, pu.SECOND):
        ctx.motion_rd_pu_device(p_luma, 2, stride, fstride, 3, mode, dev.with_fold(first.ptr), first.ptr, stream=st.cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    pu.same(first.result(RPT, shape), e2, "three launches")
    # a launch folded with what it wrote: every record ties, every byte stays
    ctx.motion_rd_pu_device(p_luma, 2, stride, fstride, 3, pu.SECOND, dev.with_fold(first.ptr), first.ptr, qp=qp, max_range=R)
    torch.cuda.synchronize()
    pu.same(first.result(RPT, shape), e2, "self-fold")
    ctx.close()


# ---- 5. bands, poisoned planes, pointers off 16, large batches, streams ------------------------------------------------------------------------------------

def test_bands_are_slices_and_an_empty_band(torch_cuda):
    torch = torch_cuda
    bd, R, qp = 10, 8, 27
    inps = inputs_of(31, R, 2)
    flat, origin, stride, fstride = plane_batch(bd, 3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma = to_dev(torch, flat)
    whole = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, 2, pu.BEST, DevInputs(torch, inps), (2, N, 85), qp, R)
    pu.same(whole, expected_batch(bd, qp, pu.BEST, inps, R), "whole")
    for rows in ((1, 2), (1, 3), (0, 1)):
        nb = (rows[1] - rows[0]) * CW
        got = run_pu(torch, ctx, d_luma, origin, stride, fstride, 3, 2, pu.BEST, DevInputs(torch, [pu.band_of(i, rows) for i in inps]), (2, nb, 85), qp, R, rows=rows)
        assert got.tobytes() == np.ascontiguousarray(whole[:, rows[0] * CW:rows[1] * CW]).tobytes(), rows
    out, dev = Guarded(torch, 4096), DevInputs(torch, inps)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_rd_pu_device(d_luma.data_ptr() + 2 * origin, 2, stride, fstride, 3, 1, dev.c, out.ptr, rows=(2, 2), qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype,bd,max_range,mode", [(np.int16, 10, 8, 4), (np.uint8, 8, 33, pu.BEST), (np.int16, 12, 64, 2)])
def test_guarded_planes_poisoned_margins_odd_origin_and_stride(torch_cuda, dtype, bd, max_range, mode):
    flat, origin, stride, fstride = plane_batch(bd, 3, dtype, extra_stride=3, shift=1, frame_gap=5, poison=77)
    assert stride % 2 == 1 and origin % 2 == 1
    inps = inputs_of(bd + max_range, max_range, 2)
    ctx = capi.Context(W, H, bd, max_frames=3)
    got = run_pu(torch_cuda, ctx, to_dev(torch_cuda, flat), origin, stride, fstride, 3, np.dtype(dtype).itemsize, mode, DevInputs(torch_cuda, inps), (2, N, 85), 22,
                 max_range)
    pu.same(got, expected_batch(bd, 22, mode, inps, max_range), (dtype.__name__, bd, max_range))
    ctx.close()


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_pointers_off_their_16_byte_alignment(torch_cuda, offset):
    """every input array and the output 4, 8, 12 bytes behind a 16-byte boundary, one at a time and all together, folding in place: the same bytes"""
    torch = torch_cuda
    bd, R, qp = 8, 8, 14
    inps = inputs_of(77, R, 1)
    flat, origin, stride, fstride = plane_batch(bd, 2)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    aligned = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, 2, pu.BEST, DevInputs(torch, inps), (1, N, 85), qp, R)
    pu.same(aligned, expected_batch(bd, qp, pu.BEST, inps, R), "aligned")
    for name in pu.Inputs._fields + (None,):
        dev = DevInputs(torch, inps, offset, only=name)
        got = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, 2, pu.BEST, dev, (1, N, 85), qp, R, out_offset=offset if name is None else 0)
        assert got.tobytes() == aligned.tobytes(), name
    held, p_fold = at_offset(torch, aligned, offset)
    again = run_pu(torch, ctx, d_luma, origin, stride, fstride, 2, 2, pu.SECOND, DevInputs(torch, inps), (1, N, 85), qp, R, fold=p_fold, out_offset=16 - offset)
    pu.same(again, expected_batch(bd, qp, pu.SECOND, inps, R, fold_into=aligned), "fold off 16")
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_more_ctus_than_the_persistent_grid(torch_cuda, max_range):
    """116 picture pairs of 9 CTUs = 1 044 CTUs in one launch: two pictures alternate and the records repeat, so pair f equals pair f - 2; the first two pairs
    equal the restatement"""
    a, b = pictures(8)[:2]
    NF = 117
    assert (NF - 1) * N > 4 * 256
    two = inputs_of(max_range, max_range, 2)
    ctx = capi.Context(W, H, 8, max_frames=NF)
    flat = np.stack([a, b] * (NF // 2) + [a]).astype(np.uint8)
    got = run_pu(torch_cuda, ctx, to_dev(torch_cuda, flat), 0, W, W * H, NF, 1, pu.BEST, DevInputs(torch_cuda, two * (NF // 2)), (NF - 1, N, 85), 22, max_range)
    exp = np.stack([pu.expected(b, a, W, H, 8, 22, pu.BEST, two[0], max_range, planes=planes_of(8, 0, max_range)),
                    pu.expected(a, b, W, H, 8, 22, pu.BEST, two[1], max_range, planes=planes_of(8, 1, max_range))])
    pu.same(got[:2], exp, "first pairs")
    first = got[:2].tobytes()
    for f in range(2, NF - 1, 2):
        assert got[f:f + 2].tobytes() == first, f
    ctx.close()


def test_two_streams_with_different_qps_ranges_and_part_modes(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, origin, stride, fstride = plane_batch(bd, 3)
    calls = [(10, 8, 1), (51, 64, pu.BEST), (27, 8, 5), (22, 33, pu.SECOND)]
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    devs = [DevInputs(torch, inputs_of(100 + i, R, 2)) for i, (_, R, _) in enumerate(calls)]
    outs = [Guarded(torch, 2 * N * 85 * 16) for _ in calls]
    torch.cuda.synchronize()
    for i, (qp, R, mode) in enumerate(calls):
        ctx.motion_rd_pu_device(d_luma.data_ptr() + 2 * origin, 2, stride, fstride, 3, mode, devs[i].c, outs[i].ptr, stream=streams[i % 2].cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    for i, (qp, R, mode) in enumerate(calls):
        pu.same(outs[i].result(RPT, (2, N, 85)), expected_batch(bd, qp, mode, inputs_of(100 + i, R, 2), R), i)
    ctx.close()


# ---- 6. the chain, the host form, the frame call -----------------------------------------------------------------------------------------------------------

def device_chain(torch, ctx, p, sb, stride, fstride, qp, R, coarse, skip_mask, stream):
    """search -> refinement -> re-pricing -> merge stages -> selection -> the RD launches -> the RD tree through the device forms on one stream, without a host
    synchronisation -> dict of Guarded outputs"""
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
    ctx.motion_rd_device(p, sb, stride, fstride, 2, rd.MERGE, g["merge"].ptr, g["rd_merge"].ptr, stream=s, qp=qp, max_range=Rm)
    inputs = ctx.rd_pu_inputs(g["priced"].ptr, g["priced_pu"].ptr, g["priced_s"].ptr, g["merge_pu"].ptr, g["merge_s"].ptr, g["mvp"].ptr, g["mvp_pu"].ptr, g["mvp_s"].ptr,
                              g["shapes"].ptr)
    ctx.motion_rd_pu_device(p, sb, stride, fstride, 2, 0, inputs, g["rd_pu"].ptr, stream=s, qp=qp, max_range=Rm)
    inputs.fold = g["rd_pu"].ptr
    for mode in (pu.BEST, pu.SECOND):
        ctx.motion_rd_pu_device(p, sb, stride, fstride, 2, mode, inputs, g["rd_pu"].ptr, stream=s, qp=qp, max_range=Rm)
    ctx.p_tree_select_rd_pu_device(g["rd_pu"].ptr, g["rd_merge"].ptr, skip_mask, 1, g["dmin"].ptr, g["dmax"].ptr, stream=s)
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("coarse", [0, 6])
def test_the_chain_on_one_stream_and_the_frame_call(torch_cuda, coarse):
    """every RD output of the chain against the restatement on the device's own intermediate records; then fhevc_p_tree_rd_frame against those pieces, with
    what it moves and launches"""
    torch = torch_cuda
    bd, R, qp, mask = 8, 8, 27, 3
    ys = frames.pan_clip(W, H, 2, seed=39, v_structure=-5, v_noise=3)
    pics = [y.astype(np.int64) for y in ys]
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=np.uint8, poison=None)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    launched = ctx.stats()["kernels_launched"]
    g = device_chain(torch, ctx, d_luma.data_ptr() + origin, 1, stride, fstride, qp, R, coarse, mask, torch.cuda.Stream())
    launched = ctx.stats()["kernels_launched"] - launched
    Rm = 64 if coarse else R
    inp = pu.Inputs(g["priced"].result(QDT, (N, 85)), g["priced_pu"].result(QDT, (N, 124)), g["priced_s"].result(QDT, (N, 384)), g["merge_pu"].result(MDT, (N, 124)),
                    g["merge_s"].result(MDT, (N, 384)), g["mvp"].result(PDT, (N, 85)), g["mvp_pu"].result(PDT, (N, 124)), g["mvp_s"].result(PDT, (N, 384)),
                    g["shapes"].result(SDT, (N, 85)))
    merge = g["merge"].result(MDT, (N, 85))
    e_merge, e_pu, emin, emax = pu.frame_records(pics[1], pics[0], W, H, bd, qp, Rm, inp, merge, mask, planes=mr.Planes(pics[0], bd, 16 if Rm <= 8 else 72))
    got_pu = g["rd_pu"].result(RPT, (N, 85))
    rd.same(g["rd_merge"].result(RDT, (N, 85)), e_merge, "rd of the merge records")
    pu.same(got_pu, e_pu, "folded")
    assert np.array_equal(g["dmin"].result(np.uint8, (N, 256)), emin) and np.array_equal(g["dmax"].result(np.uint8, (N, 256)), emax)
    valid = got_pu["part"] != 255
    assert valid.sum() > 300 and (got_pu["part"][valid] != 0).sum() > 20
    # the frame call: the same bytes from host buffers
    planes = [pel(p) for p in pics]
    before = ctx.stats()
    out = ctx.p_tree_rd_frame(planes[1][0], planes[0][0], origin=planes[0][1], stride=planes[0][2], qp=qp, search_range=R, coarse_range=coarse, skip_mask=mask,
                              with_shapes=True, with_merge=True, with_rd_merge=True, with_rd_pu=True)
    after = ctx.stats()
    names = ("dmin", "dmax", "shapes", "merge", "rd_merge", "rd_pu")
    for name, a, dt, per in zip(names, out, (np.uint8, np.uint8, SDT, MDT, RDT, RPT), (256, 256, 85, 85, 85, 85)):
        assert a.tobytes() == g[name].result(dt, (N, per)).tobytes(), name
    assert after["bytes_h2d"] - before["bytes_h2d"] == 4 * W * H and after["bytes_d2h"] - before["bytes_d2h"] == N * (2 * 256 + 4 * 85 * 16)
    assert after["kernels_launched"] - before["kernels_launched"] == launched >= 13     # the launches of the pieces, four of them RD launches
    plain = ctx.p_tree_rd_frame(planes[1][0], planes[0][0], origin=planes[0][1], stride=planes[0][2], qp=qp, search_range=R, coarse_range=coarse, skip_mask=mask)
    assert len(plain) == 2 and plain[0].tobytes() == out[0].tobytes() and plain[1].tobytes() == out[1].tobytes()
    assert ctx.stats()["bytes_d2h"] - after["bytes_d2h"] == N * 2 * 256
    ctx.close()


@pytest.mark.parametrize("max_range,mode,fold", [(8, 1, False), (64, pu.BEST, True), (8, pu.SECOND, True)])
def test_host_form_equals_device_form_and_counts_what_it_moves(torch_cuda, max_range, mode, fold):
    torch = torch_cuda
    bd, qp = 10, 22
    inp = inputs_of(3, max_range, 1)[0]
    flat, origin, stride, fstride = plane_batch(bd, 2)
    ctx = capi.Context(W, H, bd, max_frames=2)
    earlier = expected_batch(bd, qp, 0, [inp], max_range)[0] if fold else None
    held, p_fold = at_offset(torch, earlier, 0) if fold else (None, None)
    dev = run_pu(torch, ctx, to_dev(torch, flat), origin, stride, fstride, 2, 2, mode, DevInputs(torch, [inp]), (1, N, 85), qp, max_range, fold=p_fold)
    planes = [pel(p) for p in frames_of(bd, 2)]
    before = ctx.stats()
    host = ctx.motion_rd_pu(planes[1][0], planes[0][0], mode, *inp, fold=earlier, origin=planes[0][1], stride=planes[0][2], qp=qp, max_range=max_range)
    after = ctx.stats()
    assert host.tobytes() == dev[0].tobytes() and (host["part"] != 255).sum() > 100
    moved = N * (16 * (85 + 124 + 384) + 16 * (124 + 384) + 8 * (85 + 124 + 384) + 16 * 85 + (16 * 85 if fold else 0))
    assert after["bytes_h2d"] - before["bytes_h2d"] == 4 * W * H + moved and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    with pytest.raises(capi.FastHevcError):
        ctx.motion_rd_pu(planes[1][0], planes[0][0], 3, *inp, origin=planes[0][1], stride=planes[0][2], qp=qp, max_range=max_range)
    with pytest.raises(capi.FastHevcError):
        ctx.motion_rd_pu(planes[1][0], planes[0][0], mode, *inp, origin=planes[0][1], stride=planes[0][2], qp=52, max_range=max_range)
    assert ctx.stats()["kernels_launched"] == after["kernels_launched"]
    ctx.close()


# ---- 7. rejected calls, the timing slot ------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, origin, stride, fstride = plane_batch(bd, 3)
    inps = inputs_of(8, 8, 2)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev = to_dev(torch, flat), DevInputs(torch, inps)
    out = Guarded(torch, 2 * N * 85 * 16 + 64)
    torch.cuda.synchronize()
    lib = ctx.lib
    extent = 2 * N * 85 * 16
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr() + 2 * origin, sb=2, stride=stride, fs=fstride, nf=3, rb=0, re=CH, qp=30, R=8, mode=8, out=out.ptr, inputs=dict(dev.ptrs))
    ins = lambda **kw: dict(inputs=dict(dev.ptrs, **kw))
    bad = [(dict(ctx=None), None), (dict(luma=None), "argument"), (dict(inputs=None), "argument"), (ins(nodes=None), "argument"), (dict(out=None), "argument"),
           (dict(nf=1), "layout"), (dict(sb=3), "layout"), (dict(stride=W - 1), "layout"), (dict(qp=-1), "qp"), (dict(qp=52), "qp"), (dict(R=0), "max_range"),
           (dict(R=65), "max_range"), (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"), (dict(sb=1), "uint8"), (dict(fs=stride), "overlap"),
           (dict(mode=-1), "part_mode"), (dict(mode=3), "part_mode"), (dict(mode=10), "part_mode"), (dict(mode=1, **ins(pus=None, merge_pus=None, mvp_pus=None)), "two-part"),
           (ins(shapes=None), "selection"), (dict(mode=9, **ins(shapes=None)), "selection"), (dict(mode=0, **ins(pus=None)), "family"),
           (ins(pus_small=None, mvp_pus_small=None), "family"), (ins(pus_small=None, merge_pus_small=None), "family"), (dict(out=out.ptr + 2), "aligned")]
    bad += [(ins(**{name: dev.ptrs[name] + 2}), "aligned") for name in pu.Inputs._fields]
    bad += [(ins(fold=out.ptr + 2), "aligned"), (ins(fold=out.ptr + 16), "overlaps"), (ins(fold=out.ptr - 16), "overlaps"), (ins(fold=out.ptr + extent - 16), "overlaps")]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        inputs = capi.MotionRdPuInputs(**a["inputs"]) if a["inputs"] is not None else None
        return lib.fhevc_motion_rd_pu_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["mode"],
                                             C.byref(inputs) if inputs is not None else None, a["out"], None)
    for change, text in bad:
        assert call(dict(good, **change)) == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    # the host form and the frame call
    planes = [pel(p) for p in frames_of(bd, 2)]
    canary = np.full((N, 85), CANARY, np.uint8).repeat(16, axis=1).view(RPT)
    for change in (dict(qp=52), dict(max_range=0), dict(max_range=65), dict(mode=3), dict(mode=10), dict(mode=1, pus=None, merge_pus=None, mvp_pus=None)):
        res = canary.copy()
        kw = dict(dict(qp=30, max_range=8, mode=8), **{k: v for k, v in change.items() if k in ("qp", "max_range", "mode")})
        arrays = {n: getattr(inps[0], n) for n in pu.Inputs._fields if n not in change}
        inputs = capi.MotionRdPuInputs(**{n: a.ctypes.data for n, a in arrays.items()})
        rc = lib.fhevc_motion_rd_pu(ctx.h, planes[1][0].ctypes.data + 2 * planes[0][1], planes[0][0].ctypes.data + 2 * planes[0][1], planes[0][2], kw["qp"], kw["max_range"],
                                    kw["mode"], C.byref(inputs), res.ctypes.data)
        assert rc == capi.E_INVALID and res.tobytes() == canary.tobytes(), change
    maps = np.full(2 * N * 256, CANARY, np.uint8)
    for kw in (dict(qp=52), dict(skip_mask=4), dict(search_range=65), dict(search_range=9, coarse_range=3), dict(coarse_range=15)):
        a = dict(dict(qp=30, search_range=8, coarse_range=0, skip_mask=3), **kw)
        rc = lib.fhevc_p_tree_rd_frame(ctx.h, planes[1][0].ctypes.data + 2 * planes[0][1], planes[0][0].ctypes.data + 2 * planes[0][1], planes[0][2], a["qp"], a["search_range"],
                                       a["coarse_range"], None, None, a["skip_mask"], maps.ctypes.data, maps.ctypes.data + N * 256, None, None, None, None)
        assert rc == capi.E_INVALID and (maps == CANARY).all(), kw
    assert ctx.stats()["kernels_launched"] == launched
    assert call(good) == capi.OK                  # the same call with nothing wrong is accepted
    torch.cuda.synchronize()
    assert not out.untouched()
    ctx.close()


def test_slot_31_counts_one_launch_per_call_and_29_stays_untouched(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, origin, stride, fstride = plane_batch(bd, 3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, dev, out = to_dev(torch, flat), DevInputs(torch, inputs_of(8, 8, 2)), Guarded(torch, 2 * N * 85 * 16)
    dmin = Guarded(torch, 2 * N * 256)
    torch.cuda.synchronize()
    ctx.enable_kernel_timing(True)
    for s in (17, 29, 31):
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls, (R, mode) in enumerate(((8, 0), (64, 8), (8, 5)), start=1):
        ctx.motion_rd_pu_device(d_luma.data_ptr() + 2 * origin, 2, stride, fstride, 3, mode, dev.c, out.ptr, qp=30, max_range=R)
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(31)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert ctx.kernel_timing(29)[1] == 0 and ctx.kernel_timing(17)[1] == 0
    ctx.p_tree_select_rd_pu_device(out.ptr, out.ptr, 3, 2, dmin.ptr)          # the RD tree on folded records is timed as the tree
    torch.cuda.synchronize()
    assert ctx.kernel_timing(17)[1] == 1 and ctx.kernel_timing(31)[1] == 3 and ctx.kernel_timing(29)[1] == 0
    ctx.enable_kernel_timing(False)
    for s in (30, 32):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()
