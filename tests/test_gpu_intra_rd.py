"""Config 4 (P slices): the RD estimate of the intra candidate (the intra instances of k_motion_rd.hip) and the frame chain that folds it
(fhevc_p_tree_rd_intra_frame) on the MI355X, byte for byte against the restatement tests/intra_rd_ref.py, which tests/test_intra_rd_ref.py holds to closed
forms without a GPU.  Nothing is compared with the kernel's own output except where two launches must give the same bytes.

The draw's pictures are 168 x 152 (3 x 3 CTUs, ragged on both sides); the shapes are 64 x 64 and 72 x 72."""
import numpy as np
import pytest

import intra_rd_ref as ir
import motion_rd_ref as rd
from fasthevc_amd import capi
from motion_gpu_helpers import CANARY, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

PDT, NDT = ir.PDT, ir.NDT
W, H, N = ir.DRAW_W, ir.DRAW_H, ir.DRAW_N
CW, CH = 3, 3


class Guarded:
    """nbytes of device output between two canary-filled guards of 4 KiB, everything pre-filled with the canary; offset: the payload starts that many
    bytes behind a 16-byte boundary"""
    GUARD = 4096

    def __init__(self, torch, nbytes, offset=0):
        self.n, self.off = int(nbytes), self.GUARD + offset
        self.t = torch.full((self.n + 2 * self.GUARD + 16,), CANARY, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.off

    def result(self, dtype, shape):
        h = self.t.cpu().numpy()
        assert (h[:self.off] == CANARY).all() and (h[self.off + self.n:] == CANARY).all(), "a guard around the output was written"
        return h[self.off:self.off + self.n].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.t.cpu().numpy() == CANARY).all())


def at_offset(torch, a, offset):
    """the bytes of `a` on the device, starting `offset` bytes behind a 16-byte boundary -> (tensor that owns them, pointer)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros((raw.size + 32,), dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[offset:offset + raw.size] = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + offset


class Plane:
    """pictures [F, H, W] on the device in TComPicYuv's layout, as int16 or uint8 samples"""

    def __init__(self, torch, pics, dtype=np.int16):
        planes = [pel(p) for p in pics]
        self.item = np.dtype(dtype).itemsize
        self.org, self.stride, self.fstride = planes[0][1], planes[0][2], planes[0][0].size
        self.t = to_dev(torch, np.stack([p[0] for p in planes]).astype(dtype))
        self.ptr = self.t.data_ptr() + self.item * self.org
        self.frames = len(pics)


def run(torch, ctx, plane, first, qp, fold=None, merge=None, mask=0, rows=None, in_place=False, offsets=(0, 0, 0, 0), stream=None):
    """first [F, band CTUs, 85] -> the records written [F, band CTUs, 85]; the output lies between canaries (in place: the fold records lie there)"""
    held = at_offset(torch, first, offsets[0])
    held_m = at_offset(torch, merge, offsets[2]) if merge is not None else (None, None)
    out = Guarded(torch, first.size * 16, offsets[3])
    held_f = (None, None)
    if fold is not None and in_place:
        out.t[out.off:out.off + out.n] = to_dev(torch, fold)
        held_f = (None, out.ptr)
    elif fold is not None:
        held_f = at_offset(torch, fold, offsets[1])
    torch.cuda.synchronize()
    ctx.intra_rd_device(plane.ptr, plane.item, plane.stride, plane.fstride, plane.frames, held[1], out.ptr, d_fold=held_f[1], d_rd_merge=held_m[1], skip_mask=mask,
                        rows=rows, stream=stream, qp=qp)
    torch.cuda.synchronize()
    return out.result(PDT, first.shape)


def band(a, rows):
    return None if a is None else np.ascontiguousarray(a[rows[0] * CW:rows[1] * CW])


# ---- 1. the draw, byte for byte ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, dtype", [(8, np.int16), (8, np.uint8), (10, np.int16), (12, np.int16)])
def test_the_draw_plain_and_every_combination_of_gate_and_fold(torch_cuda, bd, dtype):
    torch = torch_cuda
    ctx = capi.Context(W, H, bd)
    qps = set()
    for index, (b, qp, _, _) in enumerate(ir.DRAW):
        if b != bd:
            continue
        d = ir.draw(index)
        qps.add(qp)
        plane = Plane(torch, [d["pic"]], dtype)
        first = d["first"][None]
        ir.same(run(torch, ctx, plane, first, qp)[0], d["plain"], ("plain", index))
        for fold in (None, "second", "in place"):
            for merge, masks in ((None, (0, 3)), (d["merge"], (0, 1, 2, 3))):
                for mask in masks:
                    exp = ir.gate_fold(d["plain"], d["fold"] if fold else None, merge, mask)
                    got = run(torch, ctx, plane, first, qp, d["fold"][None] if fold else None, None if merge is None else merge[None], mask, in_place=fold == "in place")
                    ir.same(got[0], exp, (index, fold, merge is not None, mask))
    assert qps == set(ir.DRAW_QPS)
    ctx.close()


# ---- 2. shapes and the closed-form pictures ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(64, 64), (72, 72), (168, 152)])
def test_shapes(torch_cuda, size):
    """64 x 64: no neighbour available anywhere; 72 x 72: only 8x8 nodes are valid in the ragged CTUs; uniform modes over 0..34 on noise with structure"""
    torch = torch_cuda
    w, h = size
    for bd, qp in ((8, 22), (10, 27), (12, 37)):
        rng = np.random.default_rng(50 + bd + w)
        yy, xx = np.mgrid[0:h, 0:w]
        pic = np.clip(((xx * 5 + yy * 3) % 200 + rng.integers(-30, 31, size=(h, w)) + 20) << (bd - 8), 0, (1 << bd) - 1).astype(np.int64)
        n = ((w + 63) // 64) * ((h + 63) // 64)
        first = ir.forced(rng.integers(0, 35, size=(n, 85)), (n, 85))
        exp = ir.plain(pic, bd, qp, first)
        assert (exp["part"] == ir.PART_INTRA).sum() >= (85 if size == (64, 64) else 100)
        if size == (72, 72):
            assert (exp["part"][1:] == ir.PART_INTRA).any() and set(ir.LEVEL_OF[np.argwhere(exp["part"][1:] == ir.PART_INTRA)[:, 1]]) == {3}
        ctx = capi.Context(w, h, bd)
        ir.same(run(torch, ctx, Plane(torch, [pic]), first[None], qp)[0], exp, (size, bd))
        ctx.close()


def test_closed_form_pictures_through_the_kernel(torch_cuda):
    torch = torch_cuda
    bd, qp = 8, 27
    lam = rd.lam_q8(qp)
    ctx = capi.Context(W, H, bd)
    yy, xx = np.mgrid[0:H, 0:W]
    flat = np.full((H, W), 1 << (bd - 1), np.int64)
    got = run(torch, ctx, Plane(torch, [flat]), ir.forced(0)[None], qp)[0]
    ir.same(got, ir.plain(flat, bd, qp, ir.forced(0)), "constant")
    v = got["part"] == ir.PART_INTRA
    ntu = np.where(ir.LEVEL_OF == 0, 4, 1)[None].repeat(N, 0)
    assert v.sum() > 300 and (got["dist"][v] == 0).all() and (got["flags"][v] == 3).all() and (got["tu_split"][v] == 0).all()
    assert (got["bits"][v] == 2 + 2 * ntu[v]).all() and (got["cost_rd"][v] == (lam * (2 + 2 * ntu[v])) >> 8).all()
    for pic, mode in (((xx * 37) % 251, 26), ((yy * 37) % 251, 10)):
        pic = pic.astype(np.int64)
        got = run(torch, ctx, Plane(torch, [pic]), ir.forced(mode)[None], qp)[0]
        ir.same(got, ir.plain(pic, bd, qp, ir.forced(mode)), mode)
        inner = got[4]   # the CTU at (1, 1): the row above and the column left of every node are available
        assert (inner["part"] == ir.PART_INTRA).all() and (inner["dist"] == 0).all() and (inner["flags"] & 3 == 3).all()
    ctx.close()


# ---- 3. bands, layouts, alignment, many CTUs, two streams ---------------------------------------------------------------------------------------------------

def test_bands_and_the_empty_band(torch_cuda):
    torch = torch_cuda
    d = ir.draw(1)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    whole = ir.gate_fold(d["plain"], d["fold"], d["merge"], 3)
    for rows in [(a, b) for a in range(CH) for b in range(a + 1, CH + 1)]:
        got = run(torch, ctx, plane, band(d["first"], rows)[None], d["qp"], band(d["fold"], rows)[None], band(d["merge"], rows)[None], 3, rows=rows)
        ir.same(got[0], band(whole, rows), rows)
        ir.same(got[0], ir.expected(d["pic"], d["bd"], d["qp"], band(d["first"], rows), band(d["fold"], rows), band(d["merge"], rows), 3, rows=rows), ("restated", rows))
    held, out = to_dev(torch, d["first"]), Guarded(torch, 4096)
    launched = ctx.stats()["kernels_launched"]
    ctx.intra_rd_device(plane.ptr, 2, plane.stride, plane.fstride, 1, held.data_ptr(), out.ptr, rows=(2, 2), qp=d["qp"])
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype", [np.int16, np.uint8])
def test_poisoned_planes_with_odd_origin_and_stride(torch_cuda, dtype):
    """the picture inside a plane of poison, its origin and stride odd: nothing outside the picture is read for its value, and the per-sample staging path
    gives the bytes of the 16-byte one"""
    torch = torch_cuda
    d = ir.draw(6 if dtype == np.uint8 else 4)
    bd = d["bd"]
    assert bd == (8 if dtype == np.uint8 else 10)
    ctx = capi.Context(W, H, bd)
    item = np.dtype(dtype).itemsize
    for seed, (stride, org) in enumerate(((W + 13, 3 * (W + 13) + 5), (W + 1, W + 1 + 1), (W, 7))):
        rng = np.random.default_rng(seed)
        buf = rng.integers(0, 1 << bd, size=org + H * stride + 64).astype(dtype)
        for y in range(H):
            buf[org + y * stride:org + y * stride + W] = d["pic"][y]
        t = to_dev(torch, buf)
        out = Guarded(torch, N * 85 * 16)
        held = to_dev(torch, d["first"])
        torch.cuda.synchronize()
        ctx.intra_rd_device(t.data_ptr() + item * org, item, stride, 0, 1, held.data_ptr(), out.ptr, qp=d["qp"])
        torch.cuda.synchronize()
        ir.same(out.result(PDT, (N, 85)), d["plain"], (stride, org))
    ctx.close()


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_pointers_off_16(torch_cuda, offset):
    torch = torch_cuda
    d = ir.draw(2)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    exp = ir.gate_fold(d["plain"], d["fold"], d["merge"], 3)
    for offsets in ((offset, 0, 0, 0), (0, offset, 0, 0), (0, 0, offset, 0), (0, 0, 0, offset), (offset, 16 - offset, offset, 16 - offset)):
        ir.same(run(torch, ctx, plane, d["first"][None], d["qp"], d["fold"][None], d["merge"][None], 3, offsets=offsets)[0], exp, offsets)
    ir.same(run(torch, ctx, plane, d["first"][None], d["qp"], d["fold"][None], d["merge"][None], 3, in_place=True, offsets=(0, 0, 0, offset))[0], exp, "in place")
    ctx.close()


def test_more_ctus_than_the_grid(torch_cuda):
    """1 044 CTUs in one launch: 116 pictures of 9 CTUs, four draws of one bit depth in turn"""
    torch = torch_cuda
    picks = [i for i, e in enumerate(ir.DRAW) if e[0] == 10][:4]
    ds = [ir.draw(i) for i in picks]
    frames = 116
    ctx = capi.Context(W, H, 10, max_frames=frames)
    plane = Plane(torch, [ds[f % 4]["pic"] for f in range(frames)])
    first = np.stack([ds[f % 4]["first"] for f in range(frames)])
    fold = np.stack([ds[f % 4]["fold"] for f in range(frames)])
    merge = np.stack([ds[f % 4]["merge"] for f in range(frames)])
    assert first.shape[0] * first.shape[1] == 1044
    qp = 27
    exp4 = [ir.expected(d["pic"], 10, qp, d["first"], d["fold"], d["merge"], 3) for d in ds]
    got = run(torch, ctx, plane, first, qp, fold, merge, 3, in_place=True)
    for f in range(frames):
        assert got[f].tobytes() == exp4[f % 4].tobytes(), f
    ctx.close()


def test_two_streams_with_different_qps(torch_cuda):
    torch = torch_cuda
    d = ir.draw(4)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    qps = (10, 37)
    exp = [ir.expected(d["pic"], d["bd"], qp, d["first"], d["fold"], d["merge"], 3) for qp in qps]
    assert exp[0].tobytes() != exp[1].tobytes()
    held, held_f, held_m = to_dev(torch, d["first"]), to_dev(torch, d["fold"]), to_dev(torch, d["merge"])
    streams = [torch.cuda.Stream() for _ in qps]
    outs = [[Guarded(torch, N * 85 * 16) for _ in range(3)] for _ in qps]
    torch.cuda.synchronize()
    for r in range(3):
        for s, qp, o in zip(streams, qps, outs):
            ctx.intra_rd_device(plane.ptr, 2, plane.stride, 0, 1, held.data_ptr(), o[r].ptr, d_fold=held_f.data_ptr(), d_rd_merge=held_m.data_ptr(), skip_mask=3,
                                stream=s.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    for e, o in zip(exp, outs):
        for r in range(3):
            ir.same(o[r].result(PDT, e.shape), e, r)
    ctx.close()


# ---- 4. chains ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, dtype", [(8, np.uint8), (10, np.int16), (12, np.int16)])
def test_first_pass_and_stage_on_one_stream(torch_cuda, bd, dtype):
    """first pass -> stage on one stream without a host synchronisation, against the oracle's first pass and the restatement"""
    torch = torch_cuda
    qp = 27
    pic = ir.draw_picture(bd, 40)
    first = ir.first_pass(pic, bd, qp)
    exp = ir.plain(pic, bd, qp, first)
    ctx = capi.Context(W, H, bd)
    plane = Plane(torch, [pic], dtype)
    d_first, out = Guarded(torch, N * 85 * 16), Guarded(torch, N * 85 * 16)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.intra_first_pass_device(plane.ptr, plane.item, plane.stride, 0, 1, d_first.ptr, stream=stream.cuda_stream, qp=qp)
    ctx.intra_rd_device(plane.ptr, plane.item, plane.stride, 0, 1, d_first.ptr, out.ptr, stream=stream.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    g = d_first.result(NDT, (N, 85))
    assert np.array_equal(g["satd"], first["satd"]) and np.array_equal(g["mode"], first["mode"])
    ir.same(out.result(PDT, (N, 85)), exp, bd)
    ctx.close()


@pytest.mark.parametrize("coarse_range", [0, 6])
def test_frame_against_its_pieces_and_its_counters(torch_cuda, coarse_range):
    bd, qp, mask = 8, 27, 3
    ref, cur = rd.draw_pictures(bd, 3)
    yy, xx = np.mgrid[0:64, 0:64]
    cur[64:128, 0:64] = 60 + (xx + yy) // 2   # a ramp the reference, texture there, does not hold: inter is dear, planar is cheap
    (bc, org, stride), (br, _, _) = pel(cur), pel(ref)
    ctx = capi.Context(W, H, bd)
    kw = dict(origin=org, stride=stride, qp=qp, search_range=8, coarse_range=coarse_range, skip_mask=mask)
    s0 = ctx.stats()
    base = ctx.p_tree_rd_frame(bc, br, with_shapes=True, with_merge=True, with_rd_merge=True, with_rd_pu=True, **kw)
    s1 = ctx.stats()
    got = ctx.p_tree_rd_intra_frame(bc, br, with_shapes=True, with_merge=True, with_rd_merge=True, with_rd_pu=True, with_first=True, **kw)
    s2 = ctx.stats()
    # the pieces: the inter chain's downloads, the first pass, the stage folding in place, the RD tree
    first = ctx.intra_first_pass(bc, org, stride, qp=qp)
    assert got[6].tobytes() == first.tobytes() and got[2].tobytes() == base[2].tobytes() and got[3].tobytes() == base[3].tobytes() and got[4].tobytes() == base[4].tobytes()
    folded = ctx.intra_rd(bc, first, fold=base[5], rd_merge=base[4], skip_mask=mask, origin=org, stride=stride, qp=qp)
    ir.same(folded, ir.expected(cur, bd, qp, first, base[5], base[4], mask), "host form against the restatement")
    assert got[5].tobytes() == folded.tobytes()
    assert (folded["part"] == ir.PART_INTRA).any() and (folded["part"] != ir.PART_INTRA).any()
    dmin, dmax = capi.p_tree_select_rd_pu(folded, base[4], mask, W, H)
    assert np.array_equal(got[0], dmin) and np.array_equal(got[1], dmax)
    # the counters: two launches more than the inter chain, the same uploads, one more array down
    assert (s2["kernels_launched"] - s1["kernels_launched"]) - (s1["kernels_launched"] - s0["kernels_launched"]) == 2
    assert s2["bytes_h2d"] - s1["bytes_h2d"] == s1["bytes_h2d"] - s0["bytes_h2d"]
    assert (s2["bytes_d2h"] - s1["bytes_d2h"]) - (s1["bytes_d2h"] - s0["bytes_d2h"]) == N * 85 * 16
    # with every first-pass record a marker the stage leaves the folded inter records as they are: the maps are fhevc_p_tree_rd_frame's
    none = np.zeros((N, 85), NDT)
    none["satd"], none["mode"] = ir.MARK, 255
    same = ctx.intra_rd(bc, none, fold=base[5], rd_merge=base[4], skip_mask=mask, origin=org, stride=stride, qp=qp)
    assert same.tobytes() == base[5].tobytes()
    dmin, dmax = capi.p_tree_select_rd_pu(same, base[4], mask, W, H)
    assert np.array_equal(base[0], dmin) and np.array_equal(base[1], dmax)
    ctx.close()


def test_host_form_equals_device_form_and_counts_what_it_moves(torch_cuda):
    torch = torch_cuda
    d = ir.draw(5)
    ctx = capi.Context(W, H, d["bd"])
    buf, org, stride = pel(d["pic"])
    for fold, merge, mask in ((None, None, 0), (d["fold"], None, 0), (d["fold"], d["merge"], 3), (None, d["merge"], 1)):
        before = ctx.stats()
        host = ctx.intra_rd(buf, d["first"], fold=fold, rd_merge=merge, skip_mask=mask, origin=org, stride=stride, qp=d["qp"])
        after = ctx.stats()
        dev = run(torch, ctx, Plane(torch, [d["pic"]]), d["first"][None], d["qp"], None if fold is None else fold[None], None if merge is None else merge[None], mask)
        assert host.tobytes() == dev[0].tobytes()
        ir.same(host, ir.gate_fold(d["plain"], fold, merge, mask), "host form")
        arrays = 1 + (fold is not None) + (merge is not None)
        assert after["bytes_h2d"] - before["bytes_h2d"] == 2 * W * H + arrays * N * 85 * 16 and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16
        assert after["kernels_launched"] - before["kernels_launched"] == 1
    ctx.close()


# ---- 5. rejected calls, the timing slot -------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing_and_the_timing_slot(torch_cuda):
    torch = torch_cuda
    d = ir.draw(1)
    ctx = capi.Context(W, H, 10, max_frames=2)
    plane = Plane(torch, [d["pic"], d["pic"]])
    first, fold, merge = (to_dev(torch, np.stack([a, a])) for a in (d["first"], d["fold"], d["merge"]))
    extent = 2 * N * 85 * 16
    out = Guarded(torch, extent + 64)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=plane.ptr, sb=2, stride=plane.stride, fs=plane.fstride, nf=2, rb=0, re=CH, qp=30, first=first.data_ptr(), fold=fold.data_ptr(),
                merge=merge.data_ptr(), mask=3, out=out.ptr)
    bad = [(dict(ctx=None), None), (dict(luma=None), "argument"), (dict(first=None), "argument"), (dict(out=None), "argument"), (dict(nf=0), "layout"), (dict(sb=3), "layout"),
           (dict(stride=W - 1), "layout"), (dict(qp=-1), "qp"), (dict(qp=52), "qp"), (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"),
           (dict(sb=1), "uint8"), (dict(mask=-1), "skip_mask"), (dict(mask=4), "skip_mask"), (dict(first=first.data_ptr() + 2), "aligned"),
           (dict(fold=fold.data_ptr() + 2), "aligned"), (dict(merge=merge.data_ptr() + 1), "aligned"), (dict(out=out.ptr + 2), "aligned"),
           (dict(fold=out.ptr + 16), "overlaps"), (dict(fold=out.ptr - 16), "overlaps"), (dict(fold=out.ptr + extent - 16), "overlaps")]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_intra_rd_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["first"], a["fold"], a["merge"], a["mask"],
                                         a["out"], None)
    for change, text in bad:
        assert call(dict(good, **change)) == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    # the host form and the frame call
    buf, org, stride = pel(d["pic"])
    res = np.full((N, 85), CANARY, np.uint8).repeat(16, axis=1).view(PDT)
    before = ctx.stats()
    for qp, mask, st in ((52, 3, stride), (30, 4, stride), (30, 3, W - 1)):
        assert lib.fhevc_intra_rd(ctx.h, buf.ctypes.data + 2 * org, st, qp, d["first"].ctypes.data, None, None, mask, res.ctypes.data) == capi.E_INVALID
    maps = np.full((2, N * 256), CANARY, np.uint8)
    for qp, mask in ((52, 3), (30, 4)):
        assert lib.fhevc_p_tree_rd_intra_frame(ctx.h, buf.ctypes.data + 2 * org, buf.ctypes.data + 2 * org, stride, qp, 8, 0, None, None, mask, maps[0].ctypes.data,
                                               maps[1].ctypes.data, None, None, None, res.ctypes.data, None) == capi.E_INVALID
    assert (res.view(np.uint8) == CANARY).all() and (maps == CANARY).all() and ctx.stats() == before
    # slot 33 counts one launch per call; 29, 31 and 17 stay untouched; 32 and 34 are no slots
    ctx.enable_kernel_timing(True)
    counts = {s: ctx.kernel_timing(s, reset=True)[1] for s in (17, 29, 31, 33)}
    for _ in range(3):
        assert call(good) == capi.OK
    torch.cuda.synchronize()
    ms, n = ctx.kernel_timing(33)
    assert n == 3 and ms > 0.0 and all(ctx.kernel_timing(s)[1] == 0 for s in (17, 29, 31)), (counts, n, ms)
    for s in (32, 34):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()
