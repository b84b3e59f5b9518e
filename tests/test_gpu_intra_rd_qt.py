"""Config 4 (P slices): the RD estimate of the intra candidate on HM's full TU tree (fhevc_intra_rd_qt* at tu_depths 3: the two further intra instances of
k_motion_rd.hip) and the frame chain that folds it (fhevc_p_tree_rd_intra_qt_frame) on the MI355X, byte for byte against the restatement
tests/intra_rd_qt_ref.py, which tests/test_intra_rd_qt_ref.py holds to intra_rd_ref, to the reference's DST and to closed forms without a GPU.  Nothing is
compared with the kernel's own output except where two launches must give the same bytes.

The draw's pictures are 168 x 152 (3 x 3 CTUs, ragged on both sides); the shapes are 64 x 64 and 72 x 72."""
import numpy as np
import pytest

import intra_rd_qt_ref as iq
import intra_rd_ref as ir
import motion_rd_ref as rd
from fasthevc_amd import capi
from motion_gpu_helpers import CANARY, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)
from test_gpu_intra_rd import CH, CW, Guarded, Plane, at_offset, band

pytestmark = pytest.mark.gpu

PDT, NDT = ir.PDT, ir.NDT
W, H, N = ir.DRAW_W, ir.DRAW_H, ir.DRAW_N
LEVEL = ir.LEVEL_OF[None].repeat(N, 0)


def run(torch, ctx, plane, first, qp, tud=3, fold=None, merge=None, mask=0, rows=None, in_place=False, offsets=(0, 0, 0, 0), stream=None):
    """first [F, band CTUs, 85] -> the records written [F, band CTUs, 85]; the output lies between canaries (in place: the fold records lie there);
    tud None: fhevc_intra_rd_device"""
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
    kw = dict(d_fold=held_f[1], d_rd_merge=held_m[1], skip_mask=mask, rows=rows, stream=stream, qp=qp)
    if tud is None:
        ctx.intra_rd_device(plane.ptr, plane.item, plane.stride, plane.fstride, plane.frames, held[1], out.ptr, **kw)
    else:
        ctx.intra_rd_qt_device(plane.ptr, plane.item, plane.stride, plane.fstride, plane.frames, held[1], tud, out.ptr, **kw)
    torch.cuda.synchronize()
    return out.result(PDT, first.shape)


# ---- 1. the draw, byte for byte ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, dtype", [(8, np.int16), (8, np.uint8), (10, np.int16), (12, np.int16)])
def test_the_draw_plain_and_every_combination_of_gate_and_fold(torch_cuda, bd, dtype):
    torch = torch_cuda
    ctx = capi.Context(W, H, bd)
    qps = set()
    for index, (b, qp, _, _) in enumerate(ir.DRAW):
        if b != bd:
            continue
        d, q = ir.draw(index), iq.draw(index)
        qps.add(qp)
        plane = Plane(torch, [d["pic"]], dtype)
        first = d["first"][None]
        got = run(torch, ctx, plane, first, qp)[0]
        iq.same(got, q["plain"], ("plain", index))
        # two depths through the new entry point: the bytes of the entry point without _qt, which are the two-depth restatement's
        two = run(torch, ctx, plane, first, qp, 2)[0]
        assert two.tobytes() == run(torch, ctx, plane, first, qp, None)[0].tobytes() == d["plain"].tobytes(), index
        assert got[:, 0].tobytes() == two[:, 0].tobytes()          # the 64x64 nodes are equal across the depth counts
        for fold in (None, "second", "in place"):
            for merge, masks in ((None, (0, 3)), (d["merge"], (0, 1, 2, 3))):
                for mask in masks:
                    exp = ir.gate_fold(q["plain"], d["fold"] if fold else None, merge, mask)
                    res = run(torch, ctx, plane, first, qp, 3, d["fold"][None] if fold else None, None if merge is None else merge[None], mask, in_place=fold == "in place")
                    iq.same(res[0], exp, (index, fold, merge is not None, mask))
    assert qps == set(ir.DRAW_QPS)
    ctx.close()


# ---- 2. shapes, the closed-form pictures, the confined bumps -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(64, 64), (72, 72)])
def test_shapes(torch_cuda, size):
    """64 x 64: no neighbour available anywhere; 72 x 72: only 8x8 nodes are valid in the ragged CTUs, and their 4x4 TUs reach the picture's edge"""
    torch = torch_cuda
    w, h = size
    for bd, qp in ((8, 22), (10, 27), (12, 37)):
        rng = np.random.default_rng(50 + bd + w)
        yy, xx = np.mgrid[0:h, 0:w]
        pic = np.clip(((xx * 5 + yy * 3) % 200 + rng.integers(-30, 31, size=(h, w)) + 20) << (bd - 8), 0, (1 << bd) - 1).astype(np.int64)
        n = ((w + 63) // 64) * ((h + 63) // 64)
        first = ir.forced(rng.integers(0, 35, size=(n, 85)), (n, 85))
        exp = iq.plain(pic, bd, qp, first, 3)
        assert (exp["part"] == ir.PART_INTRA).sum() >= (85 if size == (64, 64) else 100) and (exp["tu_split"] >> 4).any() and (exp["tu_split"][:, 21:] == 1).any()
        ctx = capi.Context(w, h, bd)
        iq.same(run(torch, ctx, Plane(torch, [pic]), first[None], qp)[0], exp, (size, bd))
        ctx.close()


def test_closed_form_pictures_and_confined_bumps_through_the_kernel(torch_cuda):
    torch = torch_cuda
    bd, qp = 8, 27
    lam = rd.lam_q8(qp)
    ctx = capi.Context(W, H, bd)
    flat = iq.constant_picture(W, H, bd, 1 << (bd - 1))
    got = run(torch, ctx, Plane(torch, [flat]), ir.forced(0)[None], qp)[0]
    iq.same(got, iq.plain(flat, bd, qp, ir.forced(0), 3), "constant")
    v = got["part"] == ir.PART_INTRA
    ntu = np.where(ir.LEVEL_OF == 0, 4, 1)[None].repeat(N, 0)
    assert v.sum() > 300 and (got["dist"][v] == 0).all() and (got["flags"][v] == 3).all() and (got["tu_split"][v] == 0).all()
    assert (got["bits"][v] == 2 + 2 * ntu[v]).all() and (got["cost_rd"][v] == (lam * (2 + 2 * ntu[v])) >> 8).all()
    for mode in (26, 10):
        pic = iq.stripes(W, H, bd, mode == 26)
        got = run(torch, ctx, Plane(torch, [pic]), ir.forced(mode)[None], qp)[0]
        iq.same(got, iq.plain(pic, bd, qp, ir.forced(mode), 3), mode)
        inner = got[4]   # the CTU at (1, 1): the row above and the column left of every TU are available
        assert (inner["part"] == ir.PART_INTRA).all() and (inner["dist"] == 0).all() and (inner["flags"] & 3 == 3).all() and (inner["tu_split"] == 0).all()
    # one checkerboard in the last 4x4 block of a 32x32, a 16x16 and an 8x8 node: tu_split known in advance (tests/test_intra_rd_qt_ref.py says why)
    for k, s, want in ((3, 32, 129), (10, 16, 129), (48, 8, 1)):
        lvl, bx, by = ir.mr.node_geometry(k)
        pic = iq.bumped(W, H, bd, 64 + bx * s + s - 4, 64 + by * s + s - 4, 60)
        got = run(torch, ctx, Plane(torch, [pic]), ir.forced(0)[None], 22)[0]
        iq.same(got, iq.plain(pic, bd, 22, ir.forced(0), 3), ("bump", k))
        assert got[4, k]["tu_split"] == want and got[4, k]["flags"] & ir.TU_SPLIT
    # a bump in every one of the 16 blocks of one 16x16 node and of the 4 of one 8x8 node, in turn: which TU sees it depends on the block
    for k, s in ((10, 16), (48, 8)):
        lvl, bx, by = ir.mr.node_geometry(k)
        for sub in range((s // 4) ** 2):
            pic = iq.bumped(W, H, bd, 64 + bx * s + (sub % (s // 4)) * 4, 64 + by * s + (sub // (s // 4)) * 4, 37)
            iq.same(run(torch, ctx, Plane(torch, [pic]), ir.forced(0)[None], 22)[0], iq.plain(pic, bd, 22, ir.forced(0), 3), ("bump", k, sub))
    ctx.close()


# ---- 3. bands, layouts, alignment, many CTUs, two streams ---------------------------------------------------------------------------------------------------

def test_bands_and_the_empty_band(torch_cuda):
    torch = torch_cuda
    d, q = ir.draw(1), iq.draw(1)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    whole = ir.gate_fold(q["plain"], d["fold"], d["merge"], 3)
    for rows in [(a, b) for a in range(CH) for b in range(a + 1, CH + 1)]:
        got = run(torch, ctx, plane, band(d["first"], rows)[None], d["qp"], 3, band(d["fold"], rows)[None], band(d["merge"], rows)[None], 3, rows=rows)
        iq.same(got[0], band(whole, rows), rows)
        iq.same(got[0], iq.expected(d["pic"], d["bd"], d["qp"], band(d["first"], rows), 3, band(d["fold"], rows), band(d["merge"], rows), 3, rows=rows), ("restated", rows))
    held, out = to_dev(torch, d["first"]), Guarded(torch, 4096)
    launched = ctx.stats()["kernels_launched"]
    ctx.intra_rd_qt_device(plane.ptr, 2, plane.stride, plane.fstride, 1, held.data_ptr(), 3, out.ptr, rows=(2, 2), qp=d["qp"])
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype", [np.int16, np.uint8])
def test_poisoned_planes_with_odd_origin_and_stride(torch_cuda, dtype):
    """the picture inside a plane of poison, its origin and stride odd: nothing outside the picture is read for its value -- the 4x4 lines included --, and
    the per-sample staging path gives the bytes of the 16-byte one"""
    torch = torch_cuda
    index = 6 if dtype == np.uint8 else 4
    d, q = ir.draw(index), iq.draw(index)
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
        ctx.intra_rd_qt_device(t.data_ptr() + item * org, item, stride, 0, 1, held.data_ptr(), 3, out.ptr, qp=d["qp"])
        torch.cuda.synchronize()
        iq.same(out.result(PDT, (N, 85)), q["plain"], (stride, org))
    ctx.close()


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_pointers_off_16(torch_cuda, offset):
    torch = torch_cuda
    d, q = ir.draw(2), iq.draw(2)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    exp = ir.gate_fold(q["plain"], d["fold"], d["merge"], 3)
    for offsets in ((offset, 0, 0, 0), (0, offset, 0, 0), (0, 0, offset, 0), (0, 0, 0, offset), (offset, 16 - offset, offset, 16 - offset)):
        iq.same(run(torch, ctx, plane, d["first"][None], d["qp"], 3, d["fold"][None], d["merge"][None], 3, offsets=offsets)[0], exp, offsets)
    iq.same(run(torch, ctx, plane, d["first"][None], d["qp"], 3, d["fold"][None], d["merge"][None], 3, in_place=True, offsets=(0, 0, 0, offset))[0], exp, "in place")
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
    exp4 = [iq.expected(d["pic"], 10, qp, d["first"], 3, d["fold"], d["merge"], 3) for d in ds]
    got = run(torch, ctx, plane, first, qp, 3, fold, merge, 3, in_place=True)
    for f in range(frames):
        assert got[f].tobytes() == exp4[f % 4].tobytes(), f
    ctx.close()


def test_two_streams_with_different_qps_and_depth_counts(torch_cuda):
    torch = torch_cuda
    d = ir.draw(4)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    legs = ((10, 3), (37, 2))
    exp = [iq.expected(d["pic"], d["bd"], qp, d["first"], tud, d["fold"], d["merge"], 3) for qp, tud in legs]
    assert exp[0].tobytes() != exp[1].tobytes()
    held, held_f, held_m = to_dev(torch, d["first"]), to_dev(torch, d["fold"]), to_dev(torch, d["merge"])
    streams = [torch.cuda.Stream() for _ in legs]
    outs = [[Guarded(torch, N * 85 * 16) for _ in range(3)] for _ in legs]
    torch.cuda.synchronize()
    for r in range(3):
        for s, (qp, tud), o in zip(streams, legs, outs):
            ctx.intra_rd_qt_device(plane.ptr, 2, plane.stride, 0, 1, held.data_ptr(), tud, o[r].ptr, d_fold=held_f.data_ptr(), d_rd_merge=held_m.data_ptr(), skip_mask=3,
                                   stream=s.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    for e, o in zip(exp, outs):
        for r in range(3):
            iq.same(o[r].result(PDT, e.shape), e, r)
    ctx.close()


# ---- 4. chains ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, dtype", [(8, np.uint8), (10, np.int16), (12, np.int16)])
def test_first_pass_and_stage_on_one_stream(torch_cuda, bd, dtype):
    """first pass -> stage on one stream without a host synchronisation, against the oracle's first pass and the restatement"""
    torch = torch_cuda
    qp = 27
    pic = ir.draw_picture(bd, 40)
    first = ir.first_pass(pic, bd, qp)
    exp = iq.plain(pic, bd, qp, first, 3)
    ctx = capi.Context(W, H, bd)
    plane = Plane(torch, [pic], dtype)
    d_first, out = Guarded(torch, N * 85 * 16), Guarded(torch, N * 85 * 16)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.intra_first_pass_device(plane.ptr, plane.item, plane.stride, 0, 1, d_first.ptr, stream=stream.cuda_stream, qp=qp)
    ctx.intra_rd_qt_device(plane.ptr, plane.item, plane.stride, 0, 1, d_first.ptr, 3, out.ptr, stream=stream.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    g = d_first.result(NDT, (N, 85))
    assert np.array_equal(g["satd"], first["satd"]) and np.array_equal(g["mode"], first["mode"])
    iq.same(out.result(PDT, (N, 85)), exp, bd)
    ctx.close()


def frame_pictures(bd):
    ref, cur = rd.draw_pictures(bd, 3)
    yy, xx = np.mgrid[0:64, 0:64]
    cur[64:128, 0:64] = 60 + (xx + yy) // 2   # a ramp the reference, texture there, does not hold: inter is dear, planar is cheap
    return ref, cur


@pytest.mark.parametrize("coarse_range", [0, 6])
def test_frame_against_its_pieces_and_its_counters(torch_cuda, coarse_range):
    """fhevc_p_tree_rd_intra_qt_frame at 3: fhevc_p_tree_rd_qt_frame's records (folded by fhevc_motion_rd_pu_qt_device at 3) taken as d_fold, in place on the
    device and through the host form; at 2 every byte of fhevc_p_tree_rd_intra_frame"""
    torch = torch_cuda
    bd, qp, mask = 8, 27, 3
    ref, cur = frame_pictures(bd)
    (bc, org, stride), (br, _, _) = pel(cur), pel(ref)
    ctx = capi.Context(W, H, bd)
    kw = dict(origin=org, stride=stride, qp=qp, search_range=8, coarse_range=coarse_range, skip_mask=mask)
    every = dict(with_shapes=True, with_merge=True, with_rd_merge=True, with_rd_pu=True)
    s0 = ctx.stats()
    base = ctx.p_tree_rd_qt_frame(bc, br, 3, **every, **kw)
    s1 = ctx.stats()
    got = ctx.p_tree_rd_intra_qt_frame(bc, br, 3, with_first=True, **every, **kw)
    s2 = ctx.stats()
    first = ctx.intra_first_pass(bc, org, stride, qp=qp)
    assert got[6].tobytes() == first.tobytes() and all(got[i].tobytes() == base[i].tobytes() for i in (2, 3, 4))
    assert (base[5]["tu_split"] >> 4).any()                     # the inter records were folded at three depths
    folded = ctx.intra_rd_qt(bc, first, 3, fold=base[5], rd_merge=base[4], skip_mask=mask, origin=org, stride=stride, qp=qp)
    iq.same(folded, iq.expected(cur, bd, qp, first, 3, base[5], base[4], mask), "host form against the restatement")
    assert got[5].tobytes() == folded.tobytes()
    wins = folded["part"] == ir.PART_INTRA
    assert wins.any() and (~wins).any() and (folded["tu_split"][wins] >> 4).any()
    # the device form, folding in place into those records
    dev = run(torch, ctx, Plane(torch, [cur]), first[None], qp, 3, base[5][None], base[4][None], mask, in_place=True)[0]
    assert dev.tobytes() == folded.tobytes()
    dmin, dmax = capi.p_tree_select_rd_pu(folded, base[4], mask, W, H)
    assert np.array_equal(got[0], dmin) and np.array_equal(got[1], dmax)
    # the counters: two launches more than the inter chain, the same uploads, one more array down
    assert (s2["kernels_launched"] - s1["kernels_launched"]) - (s1["kernels_launched"] - s0["kernels_launched"]) == 2
    assert s2["bytes_h2d"] - s1["bytes_h2d"] == s1["bytes_h2d"] - s0["bytes_h2d"]
    assert (s2["bytes_d2h"] - s1["bytes_d2h"]) - (s1["bytes_d2h"] - s0["bytes_d2h"]) == N * 85 * 16
    # two depths: every byte of the entry point without _qt
    old = ctx.p_tree_rd_intra_frame(bc, br, with_first=True, **every, **kw)
    two = ctx.p_tree_rd_intra_qt_frame(bc, br, 2, with_first=True, **every, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(old, two)) and len(old) == len(two) == 7
    assert two[5].tobytes() != got[5].tobytes()
    ctx.close()


def test_host_form_equals_device_form_and_counts_what_it_moves(torch_cuda):
    torch = torch_cuda
    d, q = ir.draw(5), iq.draw(5)
    ctx = capi.Context(W, H, d["bd"])
    buf, org, stride = pel(d["pic"])
    for fold, merge, mask in ((None, None, 0), (d["fold"], None, 0), (d["fold"], d["merge"], 3), (None, d["merge"], 1)):
        before = ctx.stats()
        host = ctx.intra_rd_qt(buf, d["first"], 3, fold=fold, rd_merge=merge, skip_mask=mask, origin=org, stride=stride, qp=d["qp"])
        after = ctx.stats()
        dev = run(torch, ctx, Plane(torch, [d["pic"]]), d["first"][None], d["qp"], 3, None if fold is None else fold[None], None if merge is None else merge[None], mask)
        assert host.tobytes() == dev[0].tobytes()
        iq.same(host, ir.gate_fold(q["plain"], fold, merge, mask), "host form")
        arrays = 1 + (fold is not None) + (merge is not None)
        assert after["bytes_h2d"] - before["bytes_h2d"] == 2 * W * H + arrays * N * 85 * 16 and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16
        assert after["kernels_launched"] - before["kernels_launched"] == 1
    two = ctx.intra_rd_qt(buf, d["first"], 2, fold=d["fold"], rd_merge=d["merge"], skip_mask=3, origin=org, stride=stride, qp=d["qp"])
    assert two.tobytes() == ctx.intra_rd(buf, d["first"], fold=d["fold"], rd_merge=d["merge"], skip_mask=3, origin=org, stride=stride, qp=d["qp"]).tobytes()
    ctx.close()


# ---- 5. rejected calls, the timing slots ------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing_and_the_timing_slots(torch_cuda):
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
                merge=merge.data_ptr(), mask=3, tud=3, out=out.ptr)
    bad = [(dict(ctx=None), None), (dict(tud=1), "tu_depths"), (dict(tud=4), "tu_depths"), (dict(tud=0), "tu_depths"), (dict(tud=-3), "tu_depths"),
           (dict(luma=None), "argument"), (dict(first=None), "argument"), (dict(out=None), "argument"), (dict(nf=0), "layout"), (dict(sb=3), "layout"),
           (dict(stride=W - 1), "layout"), (dict(qp=-1), "qp"), (dict(qp=52), "qp"), (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"),
           (dict(sb=1), "uint8"), (dict(mask=-1), "skip_mask"), (dict(mask=4), "skip_mask"), (dict(first=first.data_ptr() + 2), "aligned"),
           (dict(fold=fold.data_ptr() + 2), "aligned"), (dict(merge=merge.data_ptr() + 1), "aligned"), (dict(out=out.ptr + 2), "aligned"),
           (dict(fold=out.ptr + 16), "overlaps"), (dict(fold=out.ptr - 16), "overlaps"), (dict(fold=out.ptr + extent - 16), "overlaps")]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_intra_rd_qt_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["first"], a["fold"], a["merge"],
                                            a["mask"], a["tud"], a["out"], None)
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
    for qp, mask, st, tud in ((52, 3, stride, 3), (30, 4, stride, 3), (30, 3, W - 1, 3), (30, 3, stride, 1), (30, 3, stride, 4)):
        assert lib.fhevc_intra_rd_qt(ctx.h, buf.ctypes.data + 2 * org, st, qp, d["first"].ctypes.data, None, None, mask, tud, res.ctypes.data) == capi.E_INVALID
    maps = np.full((2, N * 256), CANARY, np.uint8)
    for qp, mask, tud in ((52, 3, 3), (30, 4, 3), (30, 3, 1), (30, 3, 4)):
        assert lib.fhevc_p_tree_rd_intra_qt_frame(ctx.h, buf.ctypes.data + 2 * org, buf.ctypes.data + 2 * org, stride, qp, 8, 0, None, None, mask, tud, maps[0].ctypes.data,
                                                  maps[1].ctypes.data, None, None, None, res.ctypes.data, None) == capi.E_INVALID
    assert (res.view(np.uint8) == CANARY).all() and (maps == CANARY).all() and ctx.stats() == before
    # slot 37 counts one launch per call at three depths, 33 at two; 17, 29, 31 and 35 stay untouched; 36 and 38 are no slots
    ctx.enable_kernel_timing(True)
    slots = (17, 29, 31, 33, 35, 37)
    for s in slots:
        ctx.kernel_timing(s, reset=True)
    for _ in range(3):
        assert call(good) == capi.OK
    torch.cuda.synchronize()
    ms, n = ctx.kernel_timing(37)
    assert n == 3 and ms > 0.0 and all(ctx.kernel_timing(s)[1] == 0 for s in (17, 29, 31, 33, 35))
    for _ in range(2):
        assert call(dict(good, tud=2)) == capi.OK
    torch.cuda.synchronize()
    assert ctx.kernel_timing(33)[1] == 2 and ctx.kernel_timing(37)[1] == 3 and all(ctx.kernel_timing(s)[1] == 0 for s in (17, 29, 31, 35))
    assert ctx.kernel_timing(37, reset=True)[1] == 3 and ctx.kernel_timing(37)[1] == 0
    for s in (36, 38):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()
