"""Config 4 (P slices): the integer motion search of the rectangular PUs (k_motion_pu.hip) on the MI355X against its numpy restatement
(tests/motion_pu_ref.py, pinned by tests/test_motion_pu_ref.py), bit for bit and field by field: distortion at the zero vector, the cheapest
vector, its distortion and its cost, for all 124 PUs of every CTU; and the 85 square nodes that ride along against fhevc_motion_search_device."""
import numpy as np
import pytest

import motion_pu_ref as pr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, Guarded, clip_planes, pel, pel_batch, same, to_dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

DT = capi.MOTION_DTYPE
NP = capi.PUS_PER_CTU


def run_dev(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, qp, R, rows=None, stream=None, with_nodes=True):
    """one launch over a device batch -> (nodes [nf - 1, band CTUs, 85] or None, pus [nf - 1, band CTUs, 124]); guards checked"""
    rows_ = rows or (0, ctx.ctus_y)
    n = (rows_[1] - rows_[0]) * ctx.ctus_x
    d_luma = to_dev(torch, flat)
    pus, nodes = Guarded(torch, max((nf - 1) * n * NP * 16, 16)), Guarded(torch, max((nf - 1) * n * 85 * 16, 16))
    torch.cuda.synchronize()
    ctx.motion_search_pu_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, pus.ptr, nodes.ptr if with_nodes else None,
                                rows=rows, stream=stream, qp=qp, search_range=R)
    torch.cuda.synchronize()
    if not with_nodes:
        assert nodes.untouched()
    return (nodes.result((nf - 1, n, 85)) if with_nodes else None), pus.result((nf - 1, n, NP))


def expected_batch(oracle, pics, bd, qp, R, sad, rows=None, ctus=None):
    """(nodes [nf - 1, band CTUs, 85], pus [nf - 1, band CTUs, 124]) of the restatement, compact over the band"""
    H, W = pics[0].shape
    cw, ch = frames.ctu_grid(W, H)
    rows = rows or (0, ch)
    sel = range(rows[0] * cw, rows[1] * cw) if ctus is None else ctus
    out = [pr.expected(oracle, pics[f], pics[f - 1], bd, qp, R, sad, ctus=sel) for f in range(1, len(pics))]
    return tuple(np.stack([o[i][rows[0] * cw:rows[1] * cw] for o in out]) for i in (0, 1))


def node_of_pu():
    return np.array([k for k, _, _ in pr.covered()])


# ---- 1. ragged picture, host form: both distortions, every bit depth, QP and range ------------------------------------------------------------------

@pytest.mark.parametrize("sad", [False, True], ids=["satd", "sad"])
@pytest.mark.parametrize("bd,qp,R", [(8, 0, 1), (8, 32, 5), (8, 51, 8), (10, 0, 5), (10, 32, 8), (10, 51, 1), (12, 0, 8), (12, 32, 1), (12, 51, 5)])
def test_ragged_picture_vs_restatement(oracle, sad, bd, qp, R):
    W, H = 176, 144   # 3 x 3 CTUs, the last column 48 wide, the last row 16 tall: valid and invalid nodes side by side at all three levels
    ys = frames.pan_clip(W, H, 2, seed=5 + bd + qp + R, v_structure=2, v_noise=-3)
    rp, cp = clip_planes(ys, bd, low_bits_seed=qp)
    (rb, org, stride), (cb, _, _) = pel(rp), pel(cp)
    ctx = capi.Context(W, H, bd)
    ctx.set_motion_distortion("sad" if sad else "satd")
    nodes, pus = ctx.motion_search_pu(cb, rb, org, stride, qp=qp, search_range=R, with_nodes=True)
    exp_nodes, exp_pus = pr.expected(oracle, cp, rp, bd, qp, R, sad)
    same(pus, exp_pus, "pus")
    same(nodes, exp_nodes, "nodes")
    same(nodes, ctx.motion_search(cb, rb, org, stride, qp=qp, search_range=R), "the existing search")
    same(ctx.motion_search_pu(cb, rb, org, stride, qp=qp, search_range=R), exp_pus, "without nodes")
    # markers exactly where the CU node's marker is, with a zero vector
    mark = pus["cost_best"] == pr.MARKER
    assert np.array_equal(mark, nodes["cost_best"][:, node_of_pu()] == pr.MARKER)
    assert (pus["satd_zero"][mark] == pr.MARKER).all() and (pus["satd_best"][mark] == pr.MARKER).all() and (pus["mvx"][mark] == 0).all() and (pus["mvy"][mark] == 0).all()
    for c, valid in ((0, 124), (2, 2 * 12 + 12 * 4), (6, 4 * 4), (8, 3 * 4)):   # whole; 48 wide: two 32x32 and twelve 16x16 nodes; 16 tall: 4 16x16; the corner: 3
        assert int((~mark[c]).sum()) == valid, c
    ctx.close()


@pytest.mark.parametrize("sad", [False, True], ids=["satd", "sad"])
def test_two_motions_in_the_halves_of_a_ctu(oracle, sad):
    """CTU 0: the left half moves by (2, -1), the right half by (-3, 2); CTU 1: top and bottom halves.  Part 0 and part 1 of the shape that cuts
    between them find those two vectors, exactly"""
    W, H, bd, qp, R = 128, 64, 10, 22, 4
    rng = np.random.default_rng(99)
    ref = rng.integers(0, 1 << bd, size=(H, W)).astype(np.int64)
    big = np.pad(ref, 8, mode="edge")
    shifted = lambda dx, dy: big[8 + dy:8 + dy + H, 8 + dx:8 + dx + W]
    a, b = shifted(2, -1), shifted(-3, 2)
    cur = a.copy()
    cur[:, 32:64] = b[:, 32:64]      # CTU 0, right half
    cur[32:, 64:] = b[32:, 64:]      # CTU 1, bottom half
    (rb, org, stride), (cb, _, _) = pel(ref), pel(cur)
    ctx = capi.Context(W, H, bd)
    ctx.set_motion_distortion("sad" if sad else "satd")
    pus = ctx.motion_search_pu(cb, rb, org, stride, qp=qp, search_range=R)
    same(pus, pr.expected(oracle, cur, ref, bd, qp, R, sad)[1])
    for ctu, shape in ((0, 1), (1, 0)):
        p0, p1 = pus[ctu, capi.motion_pu_index(0, shape, 0)], pus[ctu, capi.motion_pu_index(0, shape, 1)]
        assert (int(p0["mvx"]), int(p0["mvy"])) == (2, -1) and (int(p1["mvx"]), int(p1["mvy"])) == (-3, 2)
        assert p0["satd_best"] == 0 and p1["satd_best"] == 0 and p0["satd_zero"] > 0
    # the AMP parts on the far side of the cut see one motion only
    q = pus[0, capi.motion_pu_index(0, 4, 0)], pus[0, capi.motion_pu_index(0, 5, 1)]
    assert (int(q[0]["mvx"]), int(q[1]["mvx"])) == (2, -3) and q[0]["satd_best"] == 0 and q[1]["satd_best"] == 0
    ctx.close()


# ---- 2. device batches: square nodes, uint8 planes, layouts, bands ---------------------------------------------------------------------------------

@pytest.mark.parametrize("sad", [False, True], ids=["satd", "sad"])
def test_square_nodes_ride_along_and_uint8_planes(oracle, torch_cuda, sad):
    torch = torch_cuda
    W, H, NF, qp, R = 176, 144, 3, 30, 6
    ys = frames.pan_clip(W, H, NF, seed=4, v_structure=4, v_noise=-2)
    pics = [y.astype(np.int64) for y in ys]
    ctx = capi.Context(W, H, 8, max_frames=NF)
    ctx.set_motion_distortion("sad" if sad else "satd")
    flat, org, stride, fs = pel_batch(pics)
    nodes, pus = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R)
    exp_nodes, exp_pus = expected_batch(oracle, pics, 8, qp, R, sad)
    same(pus, exp_pus, "pus")
    same(nodes, exp_nodes, "nodes")
    # the bytes of fhevc_motion_search_device for the same arguments
    d_luma, ref_nodes = to_dev(torch, flat), Guarded(torch, nodes.size * 16)
    torch.cuda.synchronize()
    ctx.motion_search_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, ref_nodes.ptr, qp=qp, search_range=R)
    torch.cuda.synchronize()
    assert ref_nodes.result(nodes.shape).tobytes() == nodes.tobytes()
    # d_nodes NULL: the same d_pus
    _, pus_only = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R, with_nodes=False)
    assert pus_only.tobytes() == pus.tobytes()
    # uint8 planes at 8 bit equal the int16 form
    n8, p8 = run_dev(torch, ctx, np.stack(ys), 0, W, W * H, NF, 1, qp, R)
    assert p8.tobytes() == pus.tobytes() and n8.tobytes() == nodes.tobytes()
    ctx.close()


@pytest.mark.parametrize("dtype,bd,sad,shift", [(np.int16, 10, False, 1), (np.int16, 12, True, 1), (np.uint8, 8, False, 1), (np.int16, 8, True, 0), (np.uint8, 8, True, 0)])
def test_guarded_planes_poisoned_margins_both_load_paths(oracle, torch_cuda, dtype, bd, sad, shift):
    """nothing outside the picture is read for its value: margins, stride padding and the gap between frames hold poison.  shift 1: odd origin and
    odd stride, no row is aligned (the scalar staging path); shift 0: HM's alignment (the 16-byte / 8-byte staging path)"""
    torch = torch_cuda
    W, H, NF, qp, R = 176, 144, 3, 27, 7
    ys = frames.pan_clip(W, H, NF, seed=9, v_structure=-4, v_noise=6)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3 * shift, shift=shift, frame_gap=5 * shift, poison=77)
    assert (stride % 2 == 1 and origin % 2 == 1) if shift else (stride % 8 == 0 and origin % 8 == 0)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    ctx.set_motion_distortion("sad" if sad else "satd")
    nodes, pus = run_dev(torch, ctx, flat, origin, stride, fstride, NF, np.dtype(dtype).itemsize, qp, R)
    exp_nodes, exp_pus = expected_batch(oracle, pics, bd, qp, R, sad)
    same(pus, exp_pus, "pus")
    same(nodes, exp_nodes, "nodes")
    ctx.close()


def test_bands_between_canaries_and_an_empty_band(oracle, torch_cuda):
    torch = torch_cuda
    W, H, NF, qp, R = 176, 144, 3, 33, 4
    pics = clip_planes(frames.pan_clip(W, H, NF, seed=12), 10, low_bits_seed=4)
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W, H, 10, max_frames=NF)
    nodes, pus = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R)
    exp_nodes, exp_pus = expected_batch(oracle, pics, 10, qp, R, False)
    same(pus, exp_pus, "whole")
    cw = ctx.ctus_x
    for rows in ((1, 2), (0, 1), (1, 3)):     # the middle band of the 3-row picture writes exactly its extent (guards checked inside run_dev)
        n_b, p_b = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R, rows=rows)
        same(p_b, pus[:, rows[0] * cw:rows[1] * cw], rows)
        same(n_b, nodes[:, rows[0] * cw:rows[1] * cw], rows)
    # an empty band writes nothing, launches nothing and succeeds
    d_luma, out, out_n = to_dev(torch, flat), Guarded(torch, 4096), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_search_pu_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, out.ptr, out_n.ptr, rows=(2, 2), qp=qp, search_range=R)
    torch.cuda.synchronize()
    assert out.untouched() and out_n.untouched() and ctx.stats()["kernels_launched"] == launched
    # a launch is counted, and timed under which = 8
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(8, reset=True)
    big = Guarded(torch, (NF - 1) * cw * NP * 16)
    ctx.motion_search_pu_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, big.ptr, None, rows=(0, 1), qp=qp, search_range=R)
    torch.cuda.synchronize()
    ms, count = ctx.kernel_timing(8)
    assert count == 1 and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + 1 and ctx.kernel_timing(4)[1] == 0
    ctx.enable_kernel_timing(False)
    ctx.close()


# ---- 3. more CTUs than the launch grid ------------------------------------------------------------------------------------------------------------

def test_1080p_grid_stride(oracle, torch_cuda):
    """the bench geometry: three 1080p pictures = two pairs = 1020 CTUs in one launch, more than the persistent grid of three workgroups on each of
    the 256 CUs (one pair's 510 CTUs would fit into it).  The restatement on a fixed sample of CTUs that includes the last one of the launch; the
    nodes against the existing search over the whole batch"""
    torch = torch_cuda
    W, H, NF, qp, R = 1920, 1080, 3, 32, 8
    ys = frames.pan_clip(W, H, NF)
    pics = [y.astype(np.int64) for y in ys]
    planes = [frames.to_pel_plane(y, 8) for y in ys]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    assert (NF - 1) * n > 3 * 256
    nodes, pus = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R)
    d_luma, ref_nodes = to_dev(torch, flat), Guarded(torch, nodes.size * 16)
    torch.cuda.synchronize()
    ctx.motion_search_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, ref_nodes.ptr, qp=qp, search_range=R)
    torch.cuda.synchronize()
    assert ref_nodes.result(nodes.shape).tobytes() == nodes.tobytes()
    sample = {0: [0, 29, 257], 1: [3, 258, 480, 509]}     # pair 1's are work items 510 ..: past the grid; 509 = the last CTU (56 tall, bottom right)
    for f, ctus in sample.items():
        _, exp = pr.expected(oracle, pics[f + 1], pics[f], 8, qp, R, False, ctus=ctus)
        same(pus[f][ctus], exp[ctus], f)
    mark = pus["cost_best"] == pr.MARKER
    assert int((~mark).sum()) == 2 * (16 * 30 * NP + 30 * (2 * 12 + 12 * 4))   # the last row is 56 tall: its two upper 32x32 and twelve 16x16 nodes
    ctx.close()


# ---- 4. streams; the host form; rejected calls ------------------------------------------------------------------------------------------------------

def test_two_streams_in_flight_with_different_qps(torch_cuda):
    """calls on two non-blocking streams, no synchronisation between them, different QPs and ranges: each output equals that of its own synchronous
    call (the vector costs travel with the launch; nothing is shared in HBM)"""
    torch = torch_cuda
    W, H, NF = 416, 240, 3
    pics = [y.astype(np.int64) for y in frames.pan_clip(W, H, NF, seed=21, v_structure=2, v_noise=-5)]
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    calls = [(12, 8), (47, 3), (30, 8), (22, 5)]
    alone = [run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R) for qp, R in calls]
    assert not np.array_equal(alone[0][1]["cost_best"], alone[2][1]["cost_best"])
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(Guarded(torch, (NF - 1) * n * 85 * 16), Guarded(torch, (NF - 1) * n * NP * 16)) for _ in calls]
    torch.cuda.synchronize()
    for i, (qp, R) in enumerate(calls):
        ctx.motion_search_pu_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, outs[i][1].ptr, outs[i][0].ptr, stream=streams[i % 2].cuda_stream,
                                    qp=qp, search_range=R)
    torch.cuda.synchronize()
    for i in range(len(calls)):
        assert outs[i][0].result(alone[i][0].shape).tobytes() == alone[i][0].tobytes(), i
        assert outs[i][1].result(alone[i][1].shape).tobytes() == alone[i][1].tobytes(), i
    ctx.close()


def test_host_form_equals_device_form(torch_cuda):
    torch = torch_cuda
    W, H, qp = 176, 144, 29
    for bd, R, sad in ((8, 8, False), (10, 3, True), (12, 6, False)):
        pics = clip_planes(frames.pan_clip(W, H, 2, seed=60 + bd), bd, low_bits_seed=1)
        (rb, org, stride), (cb, _, _) = pel(pics[0]), pel(pics[1])
        ctx = capi.Context(W, H, bd)
        ctx.set_motion_distortion("sad" if sad else "satd")
        h_nodes, h_pus = ctx.motion_search_pu(cb, rb, org, stride, qp=qp, search_range=R, with_nodes=True)
        d_nodes, d_pus = run_dev(torch, ctx, np.stack([rb, cb]), org, stride, rb.size, 2, 2, qp, R)
        assert h_pus.tobytes() == d_pus[0].tobytes() and h_nodes.tobytes() == d_nodes[0].tobytes()
        assert (h_pus["cost_best"] != pr.MARKER).any() and (h_pus["cost_best"] == pr.MARKER).any()
        ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H = 416, 240
    ctx = capi.Context(W, H, 8)
    ctx10 = capi.Context(W, H, 10)
    n = ctx.num_ctus
    d_luma = torch.zeros((2 * W * H,), dtype=torch.int16, device="cuda")
    out, out_n = Guarded(torch, n * NP * 16), Guarded(torch, n * 85 * 16)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr(), sb=2, stride=W, fs=W * H, nf=2, rb=0, re=ctx.ctus_y, qp=32, sr=8, nodes=out_n.ptr, pus=out.ptr)
    bad = [dict(luma=None), dict(pus=None), dict(nf=1), dict(nf=0), dict(qp=-1), dict(qp=52), dict(sr=0), dict(sr=9), dict(sr=64), dict(sr=-8),
           dict(stride=W - 1), dict(rb=-1), dict(re=ctx.ctus_y + 1), dict(rb=3, re=2), dict(sb=3), dict(sb=0), dict(ctx=ctx10.h, sb=1)]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_search_pu_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["sr"], a["nodes"],
                                                 a["pus"], None)
    for change in bad:
        a = dict(good, **change)
        assert call(a) == capi.E_INVALID, change
        assert len(lib.fhevc_last_error(a["ctx"])) > 0, change          # the context says why
    assert call(dict(good, ctx=None)) == capi.E_INVALID
    torch.cuda.synchronize()
    assert out.untouched() and out_n.untouched() and ctx.stats()["kernels_launched"] == launched and ctx10.stats()["kernels_launched"] == 0
    # the host form refuses the same way
    z = np.zeros((H, W), np.int16)
    res = np.zeros((n, NP), DT)
    for qp, sr, stride in ((52, 8, W), (-1, 8, W), (32, 0, W), (32, 9, W), (32, 8, W - 1)):
        assert lib.fhevc_motion_search_pu(ctx.h, z.ctypes.data, z.ctypes.data, stride, qp, sr, None, res.ctypes.data) == capi.E_INVALID
    assert lib.fhevc_motion_search_pu(ctx.h, z.ctypes.data, z.ctypes.data, W, 32, 8, None, None) == capi.E_INVALID
    assert not res.view(np.uint8).any() and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted and writes the whole extent of both outputs
    assert call(good) == capi.OK
    torch.cuda.synchronize()
    assert not (out.result((n, NP)).view(np.uint8).reshape(-1, 16) == CANARY).all(axis=1).any()
    assert not (out_n.result((n, 85)).view(np.uint8).reshape(-1, 16) == CANARY).all(axis=1).any()
    ctx.close()
    ctx10.close()
