"""Config 4 (P slices): the integer motion search of the PUs with a 4-sample side (k_motion_pu_small.hip: AMP of the 16x16 CUs, 8x4 / 4x8 of the
8x8 CUs) on the MI355X against its numpy restatement (tests/motion_pu_small_ref.py, pinned by tests/test_motion_pu_small_ref.py), bit for bit and
field by field: distortion at the zero vector, the cheapest vector, its distortion and its cost, for all 384 PUs of every CTU."""
import numpy as np
import pytest

import motion_pu_small_ref as ps
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, Guarded, clip_planes, pel, pel_batch, same, to_dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

DT = capi.MOTION_DTYPE
NP = capi.PUS_SMALL_PER_CTU


def run_dev(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, qp, R, rows=None, stream=None):
    """one launch over a device batch -> pus [nf - 1, band CTUs, 384]; guards checked"""
    rows_ = rows or (0, ctx.ctus_y)
    n = (rows_[1] - rows_[0]) * ctx.ctus_x
    d_luma = to_dev(torch, flat)
    pus = Guarded(torch, max((nf - 1) * n * NP * 16, 16))
    torch.cuda.synchronize()
    ctx.motion_search_pu_small_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, pus.ptr, rows=rows, stream=stream, qp=qp,
                                      search_range=R)
    torch.cuda.synchronize()
    return pus.result((nf - 1, n, NP))


def expected_batch(oracle, pics, bd, qp, R, sad, rows=None, ctus=None):
    """pus [nf - 1, band CTUs, 384] of the restatement, compact over the band"""
    H, W = pics[0].shape
    cw, ch = frames.ctu_grid(W, H)
    rows = rows or (0, ch)
    sel = range(rows[0] * cw, rows[1] * cw) if ctus is None else ctus
    return np.stack([ps.expected(oracle, pics[f], pics[f - 1], bd, qp, R, sad, ctus=sel)[rows[0] * cw:rows[1] * cw] for f in range(1, len(pics))])


def node_of_pu():
    return np.array([k for k, _, _ in ps.covered()])


# ---- 1. ragged picture, host form: both distortions, every bit depth, QP and range ------------------------------------------------------------------

@pytest.mark.parametrize("sad", [False, True], ids=["satd", "sad"])
@pytest.mark.parametrize("bd,qp,R", [(8, 0, 1), (8, 51, 8), (10, 32, 8), (10, 0, 5), (12, 32, 1), (12, 51, 5)])
def test_ragged_picture_vs_restatement(oracle, sad, bd, qp, R):
    W, H = 168, 136   # 3 x 3 CTUs, the last column 40 wide, the last row 8 tall: a 16x16 node cut in half next to whole ones, 8x8 nodes alone
    ys = frames.pan_clip(W, H, 2, seed=5 + bd + qp + R, v_structure=2, v_noise=-3)
    rp, cp = clip_planes(ys, bd, low_bits_seed=qp)
    (rb, org, stride), (cb, _, _) = pel(rp), pel(cp)
    ctx = capi.Context(W, H, bd)
    ctx.set_motion_distortion("sad" if sad else "satd")
    pus = ctx.motion_search_pu_small(cb, rb, org, stride, qp=qp, search_range=R)
    same(pus, ps.expected(oracle, cp, rp, bd, qp, R, sad), "pus")
    # markers exactly where the CU node's marker is in the existing search, with a zero vector
    nodes = ctx.motion_search(cb, rb, org, stride, qp=qp, search_range=R)
    mark = pus["cost_best"] == ps.MARKER
    assert np.array_equal(mark, nodes["cost_best"][:, node_of_pu()] == ps.MARKER)
    assert (pus["satd_zero"][mark] == ps.MARKER).all() and (pus["satd_best"][mark] == ps.MARKER).all() and (pus["mvx"][mark] == 0).all() and (pus["mvy"][mark] == 0).all()
    for c, amp, small in ((0, 128, 256), (2, 64, 160), (6, 0, 32), (8, 0, 20)):   # whole; 40 wide: eight 16x16, forty 8x8 nodes; 8 tall: eight 8x8; the corner: five
        assert int((~mark[c, :128]).sum()) == amp and int((~mark[c, 128:]).sum()) == small, c
    ctx.close()


@pytest.mark.parametrize("sad", [False, True], ids=["satd", "sad"])
def test_two_motions_inside_one_cu(oracle, sad):
    """CTU 0: in every 16x16 CU the top four rows move by (2, -1), the other twelve by (-3, 2): 2NxnU finds both vectors with distortion 0 in both
    parts, where 2Nx2N cannot.  CTU 1: the same for the left four columns (nLx2N).  CTU 2 / 3: the halves of every 8x8 CU (2NxN / Nx2N)."""
    W, H, bd, qp, R = 256, 64, 10, 22, 4
    rng = np.random.default_rng(99)
    ref = rng.integers(0, 1 << bd, size=(H, W)).astype(np.int64)
    big = np.pad(ref, 8, mode="edge")
    shifted = lambda dx, dy: big[8 + dy:8 + dy + H, 8 + dx:8 + dx + W]
    va, vb = (2, -1), (-3, 2)
    a, b = shifted(*va), shifted(*vb)
    yy, xx = np.mgrid[0:H, 0:W]
    first = np.where(xx < 64, yy % 16 < 4, np.where(xx < 128, xx % 16 < 4, np.where(xx < 192, yy % 8 < 4, xx % 8 < 4)))
    cur = np.where(first, a, b)
    (rb, org, stride), (cb, _, _) = pel(ref), pel(cur)
    ctx = capi.Context(W, H, bd)
    ctx.set_motion_distortion("sad" if sad else "satd")
    pus = ctx.motion_search_pu_small(cb, rb, org, stride, qp=qp, search_range=R)
    same(pus, ps.expected(oracle, cur, ref, bd, qp, R, sad))
    nodes = ctx.motion_search(cb, rb, org, stride, qp=qp, search_range=R)
    for ctu, ks, shape in ((0, range(5, 21), 2), (1, range(5, 21), 4), (2, range(21, 85), 0), (3, range(21, 85), 1)):
        for k in ks:
            p0, p1 = pus[ctu, capi.motion_pu_small_index(k, shape, 0)], pus[ctu, capi.motion_pu_small_index(k, shape, 1)]
            assert (int(p0["mvx"]), int(p0["mvy"])) == va and (int(p1["mvx"]), int(p1["mvy"])) == vb, (ctu, k)
            assert p0["satd_best"] == 0 and p1["satd_best"] == 0 and p0["satd_zero"] > 0 and p1["satd_zero"] > 0, (ctu, k)
            assert nodes[ctu, k]["satd_best"] > 0, (ctu, k)      # one vector for the whole CU leaves a residual
    ctx.close()


# ---- 2. device batches: the existing kernels, uint8 planes, layouts, bands -------------------------------------------------------------------------

def test_sad_parts_sum_to_the_square_search_and_uint8_planes(oracle, torch_cuda):
    """SAD at 8 bit is additive: satd_zero of the two parts of every valid shape sums to satd_zero of the CU node fhevc_motion_search_device writes
    for the same planes.  uint8 planes give the bytes of the int16 form."""
    torch = torch_cuda
    W, H, NF, qp, R = 168, 136, 3, 30, 6
    ys = frames.pan_clip(W, H, NF, seed=4, v_structure=4, v_noise=-2)
    pics = [y.astype(np.int64) for y in ys]
    ctx = capi.Context(W, H, 8, max_frames=NF)
    ctx.set_motion_distortion("sad")
    flat, org, stride, fs = pel_batch(pics)
    pus = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R)
    same(pus, expected_batch(oracle, pics, 8, qp, R, True), "pus")
    d_luma, d_nodes = to_dev(torch, flat), Guarded(torch, (NF - 1) * ctx.num_ctus * 85 * 16)
    torch.cuda.synchronize()
    ctx.motion_search_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, d_nodes.ptr, qp=qp, search_range=R)
    torch.cuda.synchronize()
    nodes = d_nodes.result((NF - 1, ctx.num_ctus, 85))
    z = pus["satd_zero"].astype(np.int64)
    node_z = nodes["satd_zero"].astype(np.int64)[:, :, node_of_pu()[::2]]
    valid = node_z != ps.MARKER
    assert valid.any() and (~valid).any()
    assert np.array_equal((z[:, :, 0::2] + z[:, :, 1::2])[valid], node_z[valid])
    assert (z[:, :, 0::2][~valid] == ps.MARKER).all() and (z[:, :, 1::2][~valid] == ps.MARKER).all()
    # uint8 planes at 8 bit equal the int16 form, in both distortions
    p8 = run_dev(torch, ctx, np.stack(ys), 0, W, W * H, NF, 1, qp, R)
    assert p8.tobytes() == pus.tobytes()
    ctx.set_motion_distortion("satd")
    p8 = run_dev(torch, ctx, np.stack(ys), 0, W, W * H, NF, 1, qp, R)
    same(p8, expected_batch(oracle, pics, 8, qp, R, False), "uint8 satd")
    ctx.close()


@pytest.mark.parametrize("dtype,bd,sad,shift", [(np.int16, 10, False, 1), (np.int16, 12, True, 1), (np.uint8, 8, False, 1), (np.int16, 8, True, 0), (np.uint8, 8, True, 0),
                                                (np.int16, 12, False, 0)])
def test_guarded_planes_poisoned_margins_both_load_paths(oracle, torch_cuda, dtype, bd, sad, shift):
    """nothing outside the picture is read for its value: margins, stride padding and the gap between frames hold poison.  shift 1: odd origin and
    odd stride, no row is aligned (the scalar staging path); shift 0: HM's alignment (the 16-byte / 8-byte staging path)"""
    torch = torch_cuda
    W, H, NF, qp, R = 168, 136, 3, 27, 7
    ys = frames.pan_clip(W, H, NF, seed=9, v_structure=-4, v_noise=6)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3 * shift, shift=shift, frame_gap=5 * shift, poison=77)
    assert (stride % 2 == 1 and origin % 2 == 1) if shift else (stride % 8 == 0 and origin % 8 == 0)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    ctx.set_motion_distortion("sad" if sad else "satd")
    pus = run_dev(torch, ctx, flat, origin, stride, fstride, NF, np.dtype(dtype).itemsize, qp, R)
    same(pus, expected_batch(oracle, pics, bd, qp, R, sad), "pus")
    ctx.close()


def test_bands_between_canaries_and_an_empty_band(oracle, torch_cuda):
    torch = torch_cuda
    W, H, NF, qp, R = 168, 136, 3, 33, 4
    pics = clip_planes(frames.pan_clip(W, H, NF, seed=12), 10, low_bits_seed=4)
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W, H, 10, max_frames=NF)
    pus = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R)
    same(pus, expected_batch(oracle, pics, 10, qp, R, False), "whole")
    cw = ctx.ctus_x
    for rows in ((1, 2), (0, 1), (1, 3)):     # the middle band of the 3-row picture writes exactly its extent (guards checked inside run_dev)
        same(run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R, rows=rows), pus[:, rows[0] * cw:rows[1] * cw], rows)
    # an empty band writes nothing, launches nothing and succeeds
    d_luma, out = to_dev(torch, flat), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_search_pu_small_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, out.ptr, rows=(2, 2), qp=qp, search_range=R)
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    # a launch is counted, and timed under which = 9
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(9, reset=True)
    big = Guarded(torch, (NF - 1) * cw * NP * 16)
    ctx.motion_search_pu_small_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, big.ptr, rows=(0, 1), qp=qp, search_range=R)
    torch.cuda.synchronize()
    ms, count = ctx.kernel_timing(9)
    assert count == 1 and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + 1 and ctx.kernel_timing(8)[1] == 0 and ctx.kernel_timing(4)[1] == 0
    ctx.enable_kernel_timing(False)
    ctx.close()


# ---- 3. more CTUs than the launch grid ------------------------------------------------------------------------------------------------------------

def test_1080p_grid_stride(oracle, torch_cuda):
    """the bench geometry: four 1080p pictures = three pairs = 1530 CTUs in one launch, more than the persistent grid of four workgroups on each of
    the 256 CUs.  The restatement on a fixed sample of CTUs that includes work items past the grid and the last CTU of the launch"""
    torch = torch_cuda
    W, H, NF, qp, R = 1920, 1080, 4, 32, 8
    ys = frames.pan_clip(W, H, NF)
    pics = [y.astype(np.int64) for y in ys]
    planes = [frames.to_pel_plane(y, 8) for y in ys]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    assert (NF - 1) * n > 4 * 256
    pus = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R)
    sample = {0: [0, 257], 1: [29, 480], 2: [3, 258, 509]}     # pair 2's are work items 1020 ..: past the grid; 509 = the last CTU (56 tall, bottom right)
    for f, ctus in sample.items():
        exp = ps.expected(oracle, pics[f + 1], pics[f], 8, qp, R, False, ctus=ctus)
        same(pus[f][ctus], exp[ctus], f)
    mark = pus["cost_best"] == ps.MARKER
    assert int((~mark).sum()) == 3 * (16 * 30 * NP + 30 * (12 * 8 + 56 * 4))   # the last row is 56 tall: twelve 16x16 and fifty-six 8x8 nodes per CTU
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
    assert not np.array_equal(alone[0]["cost_best"], alone[2]["cost_best"])
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [Guarded(torch, (NF - 1) * n * NP * 16) for _ in calls]
    torch.cuda.synchronize()
    for i, (qp, R) in enumerate(calls):
        ctx.motion_search_pu_small_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, outs[i].ptr, stream=streams[i % 2].cuda_stream, qp=qp, search_range=R)
    torch.cuda.synchronize()
    for i in range(len(calls)):
        assert outs[i].result(alone[i].shape).tobytes() == alone[i].tobytes(), i
    ctx.close()


def test_host_form_equals_device_form(torch_cuda):
    torch = torch_cuda
    W, H, qp = 168, 136, 29
    for bd, R, sad in ((8, 8, False), (10, 3, True), (12, 6, False)):
        pics = clip_planes(frames.pan_clip(W, H, 2, seed=60 + bd), bd, low_bits_seed=1)
        (rb, org, stride), (cb, _, _) = pel(pics[0]), pel(pics[1])
        ctx = capi.Context(W, H, bd)
        ctx.set_motion_distortion("sad" if sad else "satd")
        h_pus = ctx.motion_search_pu_small(cb, rb, org, stride, qp=qp, search_range=R)
        d_pus = run_dev(torch, ctx, np.stack([rb, cb]), org, stride, rb.size, 2, 2, qp, R)
        assert h_pus.tobytes() == d_pus[0].tobytes()
        assert (h_pus["cost_best"] != ps.MARKER).any() and (h_pus["cost_best"] == ps.MARKER).any()
        ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H = 416, 240
    ctx = capi.Context(W, H, 8)
    ctx10 = capi.Context(W, H, 10)
    n = ctx.num_ctus
    d_luma = torch.zeros((2 * W * H,), dtype=torch.int16, device="cuda")
    out = Guarded(torch, n * NP * 16)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr(), sb=2, stride=W, fs=W * H, nf=2, rb=0, re=ctx.ctus_y, qp=32, sr=8, pus=out.ptr)
    bad = [dict(luma=None), dict(pus=None), dict(nf=1), dict(nf=0), dict(qp=-1), dict(qp=52), dict(sr=0), dict(sr=9), dict(sr=64), dict(sr=-8),
           dict(stride=W - 1), dict(rb=-1), dict(re=ctx.ctus_y + 1), dict(rb=3, re=2), dict(sb=3), dict(sb=0), dict(ctx=ctx10.h, sb=1)]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_search_pu_small_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["sr"], a["pus"], None)
    for change in bad:
        a = dict(good, **change)
        assert call(a) == capi.E_INVALID, change
        assert len(lib.fhevc_last_error(a["ctx"])) > 0, change          # the context says why
    assert call(dict(good, ctx=None)) == capi.E_INVALID
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched and ctx10.stats()["kernels_launched"] == 0
    # the host form refuses the same way
    z = np.zeros((H, W), np.int16)
    res = np.zeros((n, NP), DT)
    for qp, sr, stride in ((52, 8, W), (-1, 8, W), (32, 0, W), (32, 9, W), (32, 8, W - 1)):
        assert lib.fhevc_motion_search_pu_small(ctx.h, z.ctypes.data, z.ctypes.data, stride, qp, sr, res.ctypes.data) == capi.E_INVALID
    assert lib.fhevc_motion_search_pu_small(ctx.h, z.ctypes.data, z.ctypes.data, W, 32, 8, None) == capi.E_INVALID
    assert not res.view(np.uint8).any() and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted and writes the whole extent
    assert call(good) == capi.OK
    torch.cuda.synchronize()
    assert not (out.result((n, NP)).view(np.uint8).reshape(-1, 16) == CANARY).all(axis=1).any()
    ctx.close()
    ctx10.close()
