"""Config 4 (P slices): the quarter-sample refinement of the motion search (k_motion_refine.hip) on the MI355X against its numpy restatement
(tests/motion_refine_ref.py, pinned by tests/test_motion_refine_ref.py), bit for bit and field by field: SATD at the integer vector, the final
quarter-sample vector, its SATD and its cost, for all 85 nodes of every CTU."""
import ctypes as C

import numpy as np
import pytest

import motion_refine_ref as mr
from fasthevc_amd import capi, frames

pytestmark = pytest.mark.gpu

CANARY = 0xA5
QDT = capi.MOTION_QPEL_DTYPE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


class Guarded:
    """nbytes of device output between two canary-filled guards of 4 KiB, everything pre-filled with the canary"""
    GUARD = 4096

    def __init__(self, torch, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * self.GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + self.GUARD

    def result(self, shape):
        h = self.t.cpu().numpy()
        assert (h[:self.GUARD] == CANARY).all() and (h[self.GUARD + self.n:] == CANARY).all(), "a guard around the output was written"
        return h[self.GUARD:self.GUARD + self.n].copy().view(QDT).reshape(shape)

    def untouched(self):
        return bool((self.t.cpu().numpy() == CANARY).all())


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def same(got, exp, what=""):
    for k in QDT.names:
        assert np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:5], got[k][got[k] != exp[k]][:5], exp[k][got[k] != exp[k]][:5])


def clip_planes(ys, bd, low_bits_seed=None):
    """uint8 pictures -> ([H, W] int64 samples at bd bits per picture, with the low bits populated above 8 bit)"""
    pics = []
    for i, y in enumerate(ys):
        p = y.astype(np.int64) << (bd - 8)
        if bd > 8:
            p = p + np.random.default_rng((low_bits_seed or 0) + i).integers(0, 1 << (bd - 8), size=p.shape)
        pics.append(p)
    return pics


def pel(pic):
    """[H, W] samples -> (buffer, origin, stride) in TComPicYuv's layout (zero margins)"""
    h, w = pic.shape
    m = frames.HM_MARGIN
    buf = np.zeros((h + 2 * m, w + 2 * m), np.int16)
    buf[m:m + h, m:m + w] = pic
    return buf, m * (w + 2 * m) + m, w + 2 * m


def band_of(a, cw, rows):
    return a[rows[0] * cw:rows[1] * cw]


def random_nodes(rng, n_ctus, max_range):
    """16-byte nodes of random bytes: uniformly random int16 vectors (nearly all out of range), a third of them replaced by vectors around the
    range: inside it, on its limits and one beyond"""
    raw = rng.integers(0, 256, size=(n_ctus, 85, 16), dtype=np.uint8)
    nodes = raw.view(capi.MOTION_DTYPE).reshape(n_ctus, 85).copy()
    pick = rng.random((n_ctus, 85)) < 1 / 3
    near = rng.integers(-max_range - 1, max_range + 2, size=(2, n_ctus, 85))
    edge = rng.random((2, n_ctus, 85)) < 0.15
    near = np.where(edge, np.sign(near + 0.5).astype(np.int64) * max_range, near)
    nodes["mvx"] = np.where(pick, near[0], nodes["mvx"])
    nodes["mvy"] = np.where(pick, near[1], nodes["mvy"])
    return nodes


# ---- 1. nodes of the +-8 SATD search, every bit depth and QP, ragged picture, host form ------------------------------------------------------

@pytest.mark.parametrize("bd,qp", [(8, 22), (10, 27), (12, 32), (8, 37), (10, 0), (12, 51), (8, 0), (8, 51), (10, 37), (12, 22)])
def test_refinement_of_the_satd_search_vs_restatement(oracle, bd, qp):
    W, H, rng_ = 416, 240, 8   # ragged: last CTU column 32 wide, last row 48 tall
    ys = frames.pan_clip(W, H, 2, seed=7 + bd + qp)
    rp, cp = clip_planes(ys, bd, low_bits_seed=qp)
    (rb, org, stride), (cb, _, _) = pel(rp), pel(cp)
    ctx = capi.Context(W, H, bd)
    nodes = ctx.motion_search(cb, rb, org, stride, qp=qp, search_range=rng_)
    got = ctx.motion_refine(cb, rb, nodes, org, stride, qp=qp, max_range=rng_)
    exp = mr.expected(oracle, cb.reshape(-1), org, stride, rp, W, H, bd, qp, nodes, rng_)
    same(got, exp, (bd, qp))
    # edge-crossing nodes carry the marker exactly where the search's do.  Nothing is claimed here about leaving the integer grid: this clip moves by
    # whole samples, and at QP 51 a fractional component costs two more bits of a lambda near 68, which no node of it repays
    # (test_a_half_sample_shift_is_found_exactly_on_the_device is the case with a true sub-sample motion)
    assert np.array_equal(got["cost_best"] == mr.MARKER, nodes["cost_best"] == mr.MARKER) and (got["cost_best"][6] == mr.MARKER).any()
    ok = got["cost_best"] != mr.MARKER
    assert (got["satd_int"][ok] == nodes["satd_best"][ok]).all()      # the search's own SATD at its vector
    assert (got["cost_best"][ok] <= nodes["cost_best"][ok]).all()
    ctx.close()


@pytest.mark.parametrize("bd,fx,fy,mv", [(8, 2, 0, (3, -2)), (8, 0, 2, (-1, 4)), (10, 2, 2, (0, 0)), (12, 2, 0, (-5, 1))])
def test_a_half_sample_shift_is_found_exactly_on_the_device(oracle, bd, fx, fy, mv):
    """the cases of tests/test_motion_refine_ref.py::test_a_half_sample_shift_is_found_exactly on the kernel: the current picture IS the reference
    filtered at a half-sample offset and displaced by an integer vector; from either integer neighbour of the true position every node of every
    CTU returns the true vector with no distortion left (the restatement does, checked there on the CPU; the kernel equals the restatement)"""
    W, H, qp = 192, 128, 4
    rng = np.random.default_rng(21 + bd)     # the CPU test's content
    yy, xx = np.mgrid[0:H, 0:W]
    v = (0.5 + 0.3 * np.sin(xx / 11.0) * np.cos(yy / 7.0)) * ((1 << bd) - 1) + rng.normal(0, 40 << (bd - 8), size=(H, W))
    ref = np.clip(np.rint(v), 0, (1 << bd) - 1).astype(np.int64)
    planes = mr.Planes(ref, bd, 16)
    tx, ty = 4 * mv[0] + fx, 4 * mv[1] + fy
    y, x = planes.pad + (ty >> 2), planes.pad + (tx >> 2)
    cur = planes.planes[ty & 3][tx & 3][y:y + H, x:x + W].astype(np.int64)
    (rb, org, stride), (cb, _, _) = pel(ref), pel(cur)
    ctx = capi.Context(W, H, bd)
    n = ctx.num_ctus
    sl = mr.sqrt_lambda(oracle, qp, bd)
    for sx in ((0, 1) if fx else (0,)):
        for sy in ((0, 1) if fy else (0,)):
            nodes = np.zeros((n, 85), capi.MOTION_DTYPE)
            nodes["mvx"], nodes["mvy"] = mv[0] + sx, mv[1] + sy
            got = ctx.motion_refine(cb, rb, nodes, org, stride, qp=qp, max_range=8)
            same(got, mr.expected(oracle, cb.reshape(-1), org, stride, ref, W, H, bd, qp, nodes, 8, planes=planes), (sx, sy))
            assert (got["mvx"] == tx).all() and (got["mvy"] == ty).all() and (got["satd_best"] == 0).all() and (got["satd_int"] > 0).all()
            assert (got["cost_best"] == mr.qpel_cost(tx, ty, sl)).all()
    ctx.close()


# ---- 2. nodes of the +-64 SAD search on a fast pan: vectors that point outside the picture ---------------------------------------------------

@pytest.mark.parametrize("bd,qp,speeds", [(8, 32, (21, -37)), (10, 27, (-30, 44)), (12, 37, (40, 9))])
def test_refinement_of_the_wide_sad_search(oracle, bd, qp, speeds):
    W, H, rng_ = 416, 240, 64
    ys = frames.pan_clip(W, H, 2, seed=100 + bd, v_structure=speeds[0], v_noise=speeds[1])
    rp, cp = clip_planes(ys, bd, low_bits_seed=3)
    (rb, org, stride), (cb, _, _) = pel(rp), pel(cp)
    ctx = capi.Context(W, H, bd)
    ctx.set_motion_distortion("sad")
    nodes = ctx.motion_search(cb, rb, org, stride, qp=qp, search_range=rng_)
    got = ctx.motion_refine(cb, rb, nodes, org, stride, qp=qp, max_range=rng_)
    exp = mr.expected(oracle, cb.reshape(-1), org, stride, rp, W, H, bd, qp, nodes, rng_)
    same(got, exp, (bd, qp))
    ok = nodes["cost_best"] != mr.MARKER
    assert (np.abs(nodes["mvx"][ok]) > 8).any()
    # some node's block lands partly outside the picture: CTU column 0 with a vector to the left, or the last whole column with one to the right
    cw = (W + 63) // 64
    left = (np.arange(got.shape[0]) % cw == 0)[:, None] & ok & (nodes["mvx"] < -4)
    assert left.any() or (nodes["mvx"][ok] > 40).any()
    # the same vectors under a smaller max_range: the longer ones get the marker, the others stay as they were
    got16 = ctx.motion_refine(cb, rb, nodes, org, stride, qp=qp, max_range=16)
    far = (np.abs(nodes["mvx"].astype(int)) > 16) | (np.abs(nodes["mvy"].astype(int)) > 16) | ~ok
    assert far.any() and (~far).any() and (got16["cost_best"][far] == mr.MARKER).all() and (got16["mvx"][far] == 0).all()
    for k in QDT.names:
        assert np.array_equal(got16[k][~far], exp[k][~far]), k
    ctx.close()


# ---- 3. device batches: uint8 planes, guarded planes, synthetic nodes, bands -------------------------------------------------------------------

def run_batch(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, nodes, qp, max_range, rows=None, stream=None):
    """nodes [nf - 1, band CTUs, 85] -> the refinement's output of the same shape; guards checked"""
    d_luma, d_nodes = to_dev(torch, flat), to_dev(torch, nodes)
    out = Guarded(torch, nodes.size * 16)
    torch.cuda.synchronize()
    ctx.motion_refine_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, d_nodes.data_ptr(), out.ptr, rows=rows,
                             stream=stream, qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    return out.result(nodes.shape)


def expected_batch(oracle, pics, W, H, bd, qp, nodes, max_range, rows=None):
    """pics: [H, W] samples per frame; nodes [nf - 1, band CTUs, 85] compact over the band"""
    cw, ch = frames.ctu_grid(W, H)
    rows = rows or (0, ch)
    out = np.zeros(nodes.shape, QDT)
    for f in range(1, len(pics)):
        buf, org, stride = pel(pics[f])
        full = np.zeros((cw * ch, 85), capi.MOTION_DTYPE)
        full[rows[0] * cw:rows[1] * cw] = nodes[f - 1]
        e = mr.expected(oracle, buf.reshape(-1), org, stride, pics[f - 1], W, H, bd, qp, full, max_range, ctus=range(rows[0] * cw, rows[1] * cw))
        out[f - 1] = band_of(e, cw, rows)
    return out


@pytest.mark.parametrize("max_range", [8, 64])
def test_uint8_planes_and_synthetic_nodes(oracle, torch_cuda, max_range):
    torch = torch_cuda
    W, H, NF, qp = 416, 240, 3, 30
    ys = frames.pan_clip(W, H, NF, seed=5, v_structure=5, v_noise=-2)
    cw, ch = frames.ctu_grid(W, H)
    nodes = np.stack([random_nodes(np.random.default_rng(40 + max_range + f), cw * ch, max_range) for f in range(NF - 1)])
    ctx = capi.Context(W, H, 8, max_frames=NF)
    got = run_batch(torch, ctx, np.stack(ys), 0, W, W * H, NF, 1, nodes, qp, max_range)
    exp = expected_batch(oracle, [y.astype(np.int64) for y in ys], W, H, 8, qp, nodes, max_range)
    same(got, exp, max_range)
    out_of_range = (np.abs(nodes["mvx"].astype(int)) > max_range) | (np.abs(nodes["mvy"].astype(int)) > max_range)
    assert (got["cost_best"][out_of_range] == mr.MARKER).all() and (got["satd_int"][out_of_range] == mr.MARKER).all()
    assert (got["mvx"][out_of_range] == 0).all() and (got["mvy"][out_of_range] == 0).all()
    live = got["cost_best"] != mr.MARKER
    assert live.sum() > 100 and out_of_range.sum() > 1000
    assert (np.abs(nodes["mvx"][live]) == max_range).any() and (np.abs(nodes["mvy"][live]) == max_range).any()   # the limits themselves are inside
    # the int16 layout of the same pictures gives the same bits
    planes = [frames.to_pel_plane(y, 8) for y in ys]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    got16 = run_batch(torch, ctx, np.stack([p[0] for p in planes]), org, stride, fs, NF, 2, nodes, qp, max_range)
    same(got16, exp, "int16")
    ctx.close()


@pytest.mark.parametrize("dtype,bd,max_range", [(np.int16, 10, 8), (np.uint8, 8, 8), (np.int16, 12, 64), (np.int16, 8, 64)])
def test_guarded_planes_poisoned_margins_odd_origin_and_stride(oracle, torch_cuda, dtype, bd, max_range):
    """nothing outside the picture is read for its value: the margins, the stride padding and the gap between frames hold poison; the origin and the
    stride are odd, so no row is aligned"""
    torch = torch_cuda
    W, H, NF, qp = 200, 136, 3, 27     # ragged both ways: last column 8 wide, last row 8 tall
    ys = frames.pan_clip(W, H, NF, seed=9, v_structure=-4, v_noise=6)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3, shift=1, frame_gap=5, poison=77)
    assert stride % 2 == 1 and origin % 2 == 1
    cw, ch = frames.ctu_grid(W, H)
    rng = np.random.default_rng(bd + max_range)
    nodes = np.zeros((NF - 1, cw * ch, 85), capi.MOTION_DTYPE)
    nodes["mvx"], nodes["mvy"] = rng.integers(-max_range, max_range + 1, size=(2, NF - 1, cw * ch, 85))
    nodes["mvx"][:, :, 0], nodes["mvy"][:, :, 0] = -max_range, max_range
    ctx = capi.Context(W, H, bd, max_frames=NF)
    got = run_batch(torch, ctx, flat, origin, stride, fstride, NF, np.dtype(dtype).itemsize, nodes, qp, max_range)
    exp = expected_batch(oracle, pics, W, H, bd, qp, nodes, max_range)
    same(got, exp, (dtype.__name__, bd, max_range))
    assert (got["cost_best"] != mr.MARKER).sum() > 500
    ctx.close()


def test_bands_between_canaries_and_an_empty_band(oracle, torch_cuda):
    torch = torch_cuda
    W, H, NF, qp, max_range = 416, 240, 3, 33, 8
    ys = frames.pan_clip(W, H, NF, seed=12)
    pics = clip_planes(ys, 10, low_bits_seed=4)
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    cw, ch = frames.ctu_grid(W, H)
    rng = np.random.default_rng(8)
    full = np.zeros((NF - 1, cw * ch, 85), capi.MOTION_DTYPE)
    full["mvx"], full["mvy"] = rng.integers(-max_range, max_range + 1, size=(2, NF - 1, cw * ch, 85))
    ctx = capi.Context(W, H, 10, max_frames=NF)
    whole = run_batch(torch, ctx, flat, org, stride, fs, NF, 2, full, qp, max_range)
    same(whole, expected_batch(oracle, pics, W, H, 10, qp, full, max_range), "whole")
    for rows in ((1, 3), (0, 1), (3, 4)):
        nodes = np.ascontiguousarray(full[:, rows[0] * cw:rows[1] * cw])
        got = run_batch(torch, ctx, flat, org, stride, fs, NF, 2, nodes, qp, max_range, rows=rows)      # guards checked inside
        same(got, whole[:, rows[0] * cw:rows[1] * cw], rows)
    # an empty band writes nothing, launches nothing and succeeds
    d_luma, d_nodes, out = to_dev(torch, flat), to_dev(torch, full), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_refine_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, d_nodes.data_ptr(), out.ptr, rows=(2, 2), qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    # a launch is counted, and timed under which = 7
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(7, reset=True)
    big = Guarded(torch, (NF - 1) * cw * 85 * 16)
    ctx.motion_refine_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, d_nodes.data_ptr(), big.ptr, rows=(0, 1), qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    ms, count = ctx.kernel_timing(7)
    assert count == 1 and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + 1 and ctx.kernel_timing(4)[1] == 0
    ctx.enable_kernel_timing(False)
    ctx.close()


# ---- 4. streams -----------------------------------------------------------------------------------------------------------------------------

def test_two_streams_in_flight_with_different_qps(oracle, torch_cuda):
    """two calls on two non-blocking streams, no synchronisation between them, different QPs and ranges: each output is its own call's (the vector
    costs travel with the launch; nothing is shared in HBM)"""
    torch = torch_cuda
    W, H, NF = 416, 240, 3
    ys = frames.pan_clip(W, H, NF, seed=21, v_structure=2, v_noise=-5)
    pics = clip_planes(ys, 8)
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    cw, ch = frames.ctu_grid(W, H)
    rng = np.random.default_rng(2)
    calls = []
    for qp, max_range in ((12, 8), (47, 64), (30, 8), (22, 64)):
        nodes = np.zeros((NF - 1, cw * ch, 85), capi.MOTION_DTYPE)
        nodes["mvx"], nodes["mvy"] = rng.integers(-max_range, max_range + 1, size=(2, NF - 1, cw * ch, 85))
        calls.append((qp, max_range, nodes, expected_batch(oracle, pics, W, H, 8, qp, nodes, max_range)))
    assert not np.array_equal(calls[0][3]["cost_best"], calls[2][3]["cost_best"])
    ctx = capi.Context(W, H, 8, max_frames=NF)
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_nodes = [to_dev(torch, c[2]) for c in calls]
    outs = [Guarded(torch, c[2].size * 16) for c in calls]
    torch.cuda.synchronize()
    for i, (qp, max_range, nodes, _) in enumerate(calls):
        ctx.motion_refine_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, d_nodes[i].data_ptr(), outs[i].ptr, stream=streams[i % 2].cuda_stream,
                                 qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    for i, c in enumerate(calls):
        same(outs[i].result(c[2].shape), c[3], i)
    ctx.close()


@pytest.mark.parametrize("search", ["range8-satd", "range64-sad"])
def test_search_and_refinement_on_one_stream_without_host_synchronisation(oracle, torch_cuda, search):
    """the search writes the nodes, the refinement reads them: queued back to back on one stream (the NULL stream and a caller's), from uint8 and from
    int16 planes, the result equals the host route on the downloaded nodes"""
    torch = torch_cuda
    W, H, NF, qp = 416, 240, 3, 32
    wide = search == "range64-sad"
    rng_ = 64 if wide else 8
    ys = frames.pan_clip(W, H, NF, seed=31, v_structure=21 if wide else 3, v_noise=-37 if wide else -2)
    planes = [frames.to_pel_plane(y, 8) for y in ys]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    d8, d16 = to_dev(torch, np.stack(ys)), to_dev(torch, np.stack([p[0] for p in planes]))
    ctx = capi.Context(W, H, 8, max_frames=NF)
    if wide:
        ctx.set_motion_distortion("sad")
    n = ctx.num_ctus
    side = torch.cuda.Stream()
    results = {}
    for lname, (ptr, sb, st, fstride) in {"uint8": (d8.data_ptr(), 1, W, W * H), "int16": (d16.data_ptr() + 2 * org, 2, stride, fs)}.items():
        for sname, stream in (("null", None), ("own", side)):
            d_nodes = torch.full(((NF - 1) * n * 85 * 16,), CANARY, dtype=torch.uint8, device="cuda")
            out = Guarded(torch, (NF - 1) * n * 85 * 16)
            torch.cuda.synchronize()
            s = None if stream is None else stream.cuda_stream
            ctx.motion_search_device(ptr, sb, st, fstride, NF, d_nodes.data_ptr(), stream=s, qp=qp, search_range=rng_)
            ctx.motion_refine_device(ptr, sb, st, fstride, NF, d_nodes.data_ptr(), out.ptr, stream=s, qp=qp, max_range=rng_)
            torch.cuda.synchronize()
            results[(lname, sname)] = (d_nodes.cpu().numpy().view(capi.MOTION_DTYPE).reshape(NF - 1, n, 85), out.result((NF - 1, n, 85)))
    nodes, _ = results[("int16", "null")]
    assert (nodes["mvx"] != 0).any()
    exp = expected_batch(oracle, [y.astype(np.int64) for y in ys], W, H, 8, qp, nodes, rng_)
    for key, (gn, gq) in results.items():
        assert all(np.array_equal(gn[k], nodes[k]) for k in capi.MOTION_DTYPE.names), key
        same(gq, exp, key)
    ctx.close()


# ---- 5. the host form against the device form; rejected calls ----------------------------------------------------------------------------------

def test_host_form_equals_device_form(torch_cuda):
    torch = torch_cuda
    W, H, qp = 416, 240, 29
    for bd, max_range in ((8, 8), (10, 64), (12, 8)):
        ys = frames.pan_clip(W, H, 2, seed=60 + bd)
        pics = clip_planes(ys, bd, low_bits_seed=1)
        (rb, org, stride), (cb, _, _) = pel(pics[0]), pel(pics[1])
        ctx = capi.Context(W, H, bd)
        n = ctx.num_ctus
        rng = np.random.default_rng(bd)
        nodes = np.zeros((n, 85), capi.MOTION_DTYPE)
        nodes["mvx"], nodes["mvy"] = rng.integers(-max_range - 2, max_range + 3, size=(2, n, 85))
        host = ctx.motion_refine(cb, rb, nodes, org, stride, qp=qp, max_range=max_range)
        dev = run_batch(torch, ctx, np.stack([rb, cb]), org, stride, rb.size, 2, 2, nodes[None], qp, max_range)[0]
        same(host, dev, bd)
        assert (host["cost_best"] != mr.MARKER).any() and (host["cost_best"] == mr.MARKER).any()
        ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H = 416, 240
    ctx = capi.Context(W, H, 8)
    ctx10 = capi.Context(W, H, 10)
    n = ctx.num_ctus
    d_luma = torch.zeros((2 * W * H,), dtype=torch.int16, device="cuda")
    d_nodes = torch.zeros((n * 85 * 16,), dtype=torch.uint8, device="cuda")
    out = Guarded(torch, n * 85 * 16)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr(), sb=2, stride=W, fs=W * H, nf=2, rb=0, re=ctx.ctus_y, qp=32, mr=8, nodes=d_nodes.data_ptr(), out=out.ptr)
    bad = [dict(luma=None), dict(nodes=None), dict(out=None), dict(nf=1), dict(nf=0), dict(qp=-1), dict(qp=52), dict(mr=0), dict(mr=65), dict(mr=-8),
           dict(stride=W - 1), dict(rb=-1), dict(re=ctx.ctus_y + 1), dict(rb=3, re=2), dict(sb=3), dict(sb=0), dict(ctx=ctx10.h, sb=1)]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_refine_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["mr"], a["nodes"],
                                              a["out"], None)
    for change in bad:
        a = dict(good, **change)
        assert call(a) == capi.E_INVALID, change
        assert len(lib.fhevc_last_error(a["ctx"])) > 0, change          # the context says why
    assert call(dict(good, ctx=None)) == capi.E_INVALID
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched and ctx10.stats()["kernels_launched"] == 0
    # the host form refuses the same way
    z = np.zeros((H, W), np.int16)
    nodes, res = np.zeros((n, 85), capi.MOTION_DTYPE), np.zeros((n, 85), QDT)
    for qp, mrange, stride in ((52, 8, W), (-1, 8, W), (32, 0, W), (32, 65, W), (32, 8, W - 1)):
        assert lib.fhevc_motion_refine(ctx.h, z.ctypes.data, z.ctypes.data, stride, qp, mrange, nodes.ctypes.data, res.ctypes.data) == capi.E_INVALID
    assert lib.fhevc_motion_refine(ctx.h, z.ctypes.data, z.ctypes.data, W, 32, 8, None, res.ctypes.data) == capi.E_INVALID
    assert not res.view(np.uint8).any() and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted and writes the whole extent
    assert call(good) == capi.OK
    torch.cuda.synchronize()
    r = out.result((n, 85))
    assert not (r.view(np.uint8).reshape(-1, 16) == CANARY).all(axis=1).any()
    ctx.close()
    ctx10.close()


# ---- 6. a 1080p pair, whole picture ------------------------------------------------------------------------------------------------------------

def test_1080p_pair_whole_picture(oracle, torch_cuda):
    torch = torch_cuda
    W, H, qp, rng_ = 1920, 1080, 32, 8
    ys = frames.pan_clip(W, H, 2)
    pics = clip_planes(ys, 8)
    planes = [frames.to_pel_plane(y, 8) for y in ys]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 8, max_frames=2)
    n = ctx.num_ctus
    d16 = to_dev(torch, np.stack([p[0] for p in planes]))
    d_nodes = torch.zeros((n * 85 * 16,), dtype=torch.uint8, device="cuda")
    out = Guarded(torch, n * 85 * 16)
    torch.cuda.synchronize()
    ctx.motion_search_device(d16.data_ptr() + 2 * org, 2, stride, fs, 2, d_nodes.data_ptr(), qp=qp, search_range=rng_)
    ctx.motion_refine_device(d16.data_ptr() + 2 * org, 2, stride, fs, 2, d_nodes.data_ptr(), out.ptr, qp=qp, max_range=rng_)
    torch.cuda.synchronize()
    nodes = d_nodes.cpu().numpy().view(capi.MOTION_DTYPE).reshape(1, n, 85)
    got = out.result((1, n, 85))
    exp = expected_batch(oracle, pics, W, H, 8, qp, nodes, rng_)
    same(got, exp, "1080p")
    ok = got["cost_best"] != mr.MARKER
    assert ok.sum() == 16 * 30 * 85 + 30 * (2 + 12 + 56)   # every node of the 16 whole CTU rows; the last row is 56 tall: 2 + 12 + 56 nodes per CTU
    assert (got["cost_best"][ok] < nodes["cost_best"][ok]).any()
    ctx.close()
