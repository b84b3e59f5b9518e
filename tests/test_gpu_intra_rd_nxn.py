"""Config 4 (P slices): the intra RD stage with the NxN candidate of the 8x8 nodes (fhevc_intra_rd_nxn*: the two NxN instances of k_motion_rd.hip) and
the frame chain that folds it (fhevc_p_tree_rd_intra_nxn_frame) on the MI355X, byte for byte against the restatement tests/intra_rd_nxn_ref.py, which
tests/test_intra_rd_nxn_ref.py holds to intra_rd_qt_ref and to closed forms without a GPU.  Nothing is compared with the kernel's own output except where two
launches must give the same bytes.

The draw's pictures are 168 x 152 (3 x 3 CTUs, ragged on both sides); the shapes are 64 x 64 and 72 x 72."""
import numpy as np
import pytest

import intra_rd_nxn_ref as nx
import intra_rd_qt_ref as iq
import intra_rd_ref as ir
import motion_rd_ref as rd
from fasthevc_amd import capi
from motion_gpu_helpers import CANARY, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)
from test_gpu_intra_rd import CH, CW, Guarded, Plane, at_offset, band
from test_gpu_intra_rd_qt import frame_pictures

pytestmark = pytest.mark.gpu

PDT, NDT, XDT = nx.PDT, nx.NDT, nx.XDT
W, H, N = ir.DRAW_W, ir.DRAW_H, ir.DRAW_N


def run(torch, ctx, plane, first, first4, qp, fold=None, merge=None, mask=0, rows=None, in_place=False, offsets=(0, 0, 0, 0), stream=None, with_nxn=True, off4=0, offx=0):
    """first [F, band CTUs, 85], first4 [F, band CTUs, 256] or None -> (the records written [F, band CTUs, 85], the NxN records [F, band CTUs, 64] or None);
    both outputs lie between canaries (in place: the fold records lie in the first)"""
    held = at_offset(torch, first, offsets[0])
    held4 = at_offset(torch, first4, off4) if first4 is not None else (None, None)
    held_m = at_offset(torch, merge, offsets[2]) if merge is not None else (None, None)
    out = Guarded(torch, first.size * 16, offsets[3])
    outx = Guarded(torch, first.size // 85 * 64 * 16, offx) if with_nxn else None
    held_f = (None, None)
    if fold is not None and in_place:
        out.t[out.off:out.off + out.n] = to_dev(torch, fold)
        held_f = (None, out.ptr)
    elif fold is not None:
        held_f = at_offset(torch, fold, offsets[1])
    torch.cuda.synchronize()
    ctx.intra_rd_nxn_device(plane.ptr, plane.item, plane.stride, plane.fstride, plane.frames, held[1], held4[1], out.ptr, outx.ptr if with_nxn else None, d_fold=held_f[1],
                            d_rd_merge=held_m[1], skip_mask=mask, rows=rows, stream=stream, qp=qp)
    torch.cuda.synchronize()
    shape = first.shape[:-1]
    return out.result(PDT, first.shape), outx.result(XDT, shape + (64,)) if with_nxn else None


# ---- 1. the draw, byte for byte ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, dtype", [(8, np.int16), (8, np.uint8), (10, np.int16), (12, np.int16)])
def test_the_draw_both_outputs_plain_and_every_combination_of_gate_and_fold(torch_cuda, bd, dtype):
    torch = torch_cuda
    ctx = capi.Context(W, H, bd)
    taken = 0
    for index, (b, qp, _, _) in enumerate(ir.DRAW):
        if b != bd:
            continue
        d = nx.draw(index)
        plane = Plane(torch, [d["pic"]], dtype)
        first, first4 = d["first"][None], d["first4"][None]
        got, gx = run(torch, ctx, plane, first, first4, qp)
        nx.same(gx[0], d["nxn"], ("nxn", index))
        nx.same(got[0], d["plain"], ("plain", index))
        taken += int((got[0]["part"] == nx.PART_NXN).sum())
        nox, none = run(torch, ctx, plane, first, first4, qp, with_nxn=False)
        assert none is None and nox.tobytes() == got.tobytes()
        for fold in (None, "second", "in place"):
            for merge, masks in ((None, (0, 3)), (d["merge"], (0, 1, 2, 3))):
                for mask in masks:
                    exp = ir.gate_fold(d["plain"], d["fold"] if fold else None, merge, mask)
                    res, rx = run(torch, ctx, plane, first, first4, qp, d["fold"][None] if fold else None, None if merge is None else merge[None], mask, in_place=fold == "in place")
                    nx.same(res[0], exp, (index, fold, merge is not None, mask))
                    assert rx.tobytes() == gx.tobytes()          # the NxN records do not depend on the gate, the fold or the choice
    assert taken > 100
    ctx.close()


@pytest.mark.parametrize("index", [0, 1, 2])
def test_without_first4_it_is_the_three_depth_stage_and_the_own_mode_never_wins(torch_cuda, index):
    torch = torch_cuda
    d, q = nx.draw(index), iq.draw(index)
    ctx = capi.Context(W, H, d["bd"])
    ctx.enable_kernel_timing(True)
    for s in (37, 39):
        ctx.kernel_timing(s, reset=True)
    plane = Plane(torch, [d["pic"]])
    first = d["first"][None]
    exp = ir.gate_fold(q["plain"], d["fold"], d["merge"], 3)
    got, _ = run(torch, ctx, plane, first, None, d["qp"], d["fold"][None], d["merge"][None], 3, with_nxn=False)
    nx.same(got[0], exp, "no first4")
    out = Guarded(torch, N * 85 * 16)
    hf, hfo, hm = to_dev(torch, d["first"]), to_dev(torch, d["fold"]), to_dev(torch, d["merge"])
    torch.cuda.synchronize()
    ctx.intra_rd_qt_device(plane.ptr, 2, plane.stride, 0, 1, hf.data_ptr(), 3, out.ptr, d_fold=hfo.data_ptr(), d_rd_merge=hm.data_ptr(), skip_mask=3, qp=d["qp"])
    torch.cuda.synchronize()
    assert out.result(PDT, (N, 85)).tobytes() == got[0].tobytes()
    assert ctx.kernel_timing(37)[1] == 2 and ctx.kernel_timing(39)[1] == 0      # the launch itself is the mirrored call's
    # the node's own mode four times: NxN is dearer by lam (3 bits(m) - 1), every byte is the stage's without first4
    own = nx.own_first4(d["first"])
    got2, gx = run(torch, ctx, plane, first, own[None], d["qp"], d["fold"][None], d["merge"][None], 3)
    assert got2.tobytes() == got.tobytes() and ctx.kernel_timing(39)[1] == 1
    nx.same(gx[0], nx.candidates(d["pic"], d["bd"], d["qp"], own), "own mode")
    ctx.close()


# ---- 2. pictures with values known in advance, shapes ------------------------------------------------------------------------------------------------------

def test_the_constant_and_the_quadrant_stripe_pictures(torch_cuda):
    torch = torch_cuda
    for bd, qp in ((8, 27), (10, 32), (12, 22)):
        lam = rd.lam_q8(qp)
        ctx = capi.Context(64, 64, bd)
        flat = iq.constant_picture(64, 64, bd, 1 << (bd - 1))
        got, gx = run(torch, ctx, Plane(torch, [flat]), ir.forced(0, (1, 1, 85)), ir.forced(0, (1, 1, 256)), qp)
        assert (gx["dist"] == 0).all() and (gx["bits"] == 12).all() and (gx["cost_rd"] == (12 * lam) >> 8).all() and (gx["flags"] == 7).all() and (gx["cbf"] == 0).all()
        assert (got[0, 0, 21:]["part"] == ir.PART_INTRA).all() and (got[0, 0, 21:]["cost_rd"] == (4 * lam) >> 8).all()
        pic = nx.quadrant_stripes(64, 64, bd, 8, 8)
        first4 = ir.forced(0, (1, 256))
        first4["mode"][0, nx.units(9)] = nx.STRIPE_MODES
        for m in (0, 1, 10, 26, 18, 34):
            first = ir.forced(m, (1, 85))
            got, gx = run(torch, ctx, Plane(torch, [pic]), first[None], first4[None], qp)
            ep, ex = nx.plain(pic, bd, qp, first, first4)
            nx.same(got[0], ep, ("stripes", bd, m))
            nx.same(gx[0], ex, ("stripes nxn", bd, m))
            r = got[0, 0, 21 + 9]
            assert (r["part"], r["dist"], r["cost_rd"], r["bits"], r["flags"], r["tu_split"], tuple(r["pad"])) == (nx.PART_NXN, 0, (22 * lam) >> 8, 22, 7, 1, (0, 0))
            assert tuple(gx[0, 0, 9]["modes"]) == nx.STRIPE_MODES
        ctx.close()


@pytest.mark.parametrize("size", [(64, 64), (72, 72)])
def test_shapes(torch_cuda, size):
    """64 x 64: no neighbour available anywhere; 72 x 72: the column and the row of 8x8 nodes at 64 are priced, their 4x4 PUs reach the picture's edge"""
    torch = torch_cuda
    w, h = size
    for bd, qp in ((8, 22), (10, 27), (12, 37)):
        rng = np.random.default_rng(60 + bd + w)
        yy, xx = np.mgrid[0:h, 0:w]
        pic = np.clip(((xx * 5 + yy * 3) % 200 + rng.integers(-30, 31, size=(h, w)) + 20) << (bd - 8), 0, (1 << bd) - 1).astype(np.int64)
        n = ((w + 63) // 64) * ((h + 63) // 64)
        first = ir.forced(rng.integers(0, 35, size=(n, 85)), (n, 85))
        first4 = ir.forced(rng.integers(0, 35, size=(n, 256)), (n, 256))
        ep, ex = nx.plain(pic, bd, qp, first, first4)
        assert (ex["cost_rd"] != nx.MARK).sum() == (64 if size == (64, 64) else 81) and (ep["part"] == nx.PART_NXN).sum() >= 2
        ctx = capi.Context(w, h, bd)
        got, gx = run(torch, ctx, Plane(torch, [pic]), first[None], first4[None], qp)
        nx.same(gx[0], ex, (size, bd))
        nx.same(got[0], ep, (size, bd))
        ctx.close()


# ---- 3. bands, layouts, alignment, many CTUs, two streams ---------------------------------------------------------------------------------------------------

def test_bands_and_the_empty_band(torch_cuda):
    torch = torch_cuda
    d = nx.draw(1)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    whole = ir.gate_fold(d["plain"], d["fold"], d["merge"], 3)
    for rows in [(a, b) for a in range(CH) for b in range(a + 1, CH + 1)]:
        got, gx = run(torch, ctx, plane, band(d["first"], rows)[None], band(d["first4"], rows)[None], d["qp"], band(d["fold"], rows)[None], band(d["merge"], rows)[None], 3, rows=rows)
        nx.same(got[0], band(whole, rows), rows)
        nx.same(gx[0], band(d["nxn"], rows), rows)
    held, held4, out, outx = to_dev(torch, d["first"]), to_dev(torch, d["first4"]), Guarded(torch, 4096), Guarded(torch, 4096)
    launched = ctx.stats()["kernels_launched"]
    ctx.intra_rd_nxn_device(plane.ptr, 2, plane.stride, plane.fstride, 1, held.data_ptr(), held4.data_ptr(), out.ptr, outx.ptr, rows=(2, 2), qp=d["qp"])
    torch.cuda.synchronize()
    assert out.untouched() and outx.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype", [np.int16, np.uint8])
def test_poisoned_planes_with_odd_origin_and_stride(torch_cuda, dtype):
    torch = torch_cuda
    index = 6 if dtype == np.uint8 else 4
    d = nx.draw(index)
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
        out, outx = Guarded(torch, N * 85 * 16), Guarded(torch, N * 64 * 16)
        held, held4 = to_dev(torch, d["first"]), to_dev(torch, d["first4"])
        torch.cuda.synchronize()
        ctx.intra_rd_nxn_device(t.data_ptr() + item * org, item, stride, 0, 1, held.data_ptr(), held4.data_ptr(), out.ptr, outx.ptr, qp=d["qp"])
        torch.cuda.synchronize()
        nx.same(out.result(PDT, (N, 85)), d["plain"], (stride, org))
        nx.same(outx.result(XDT, (N, 64)), d["nxn"], (stride, org))
    ctx.close()


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_pointers_off_16(torch_cuda, offset):
    torch = torch_cuda
    d = nx.draw(2)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    exp = ir.gate_fold(d["plain"], d["fold"], d["merge"], 3)
    for off4, offx, offo in ((offset, 0, 0), (0, offset, 0), (0, 0, offset), (offset, 16 - offset, offset)):
        got, gx = run(torch, ctx, plane, d["first"][None], d["first4"][None], d["qp"], d["fold"][None], d["merge"][None], 3, offsets=(0, 0, 0, offo), off4=off4, offx=offx)
        nx.same(got[0], exp, (off4, offx, offo))
        nx.same(gx[0], d["nxn"], (off4, offx, offo))
    got, gx = run(torch, ctx, plane, d["first"][None], d["first4"][None], d["qp"], d["fold"][None], d["merge"][None], 3, in_place=True, offsets=(0, 0, 0, offset), off4=offset,
                  offx=offset)
    nx.same(got[0], exp, "in place")
    nx.same(gx[0], d["nxn"], "in place")
    ctx.close()


def test_more_ctus_than_the_grid(torch_cuda):
    """1 044 CTUs in one launch: 116 pictures of 9 CTUs, four draws of one bit depth in turn"""
    torch = torch_cuda
    picks = [i for i, e in enumerate(ir.DRAW) if e[0] == 10][:4]
    ds = [nx.draw(i) for i in picks]
    frames = 116
    ctx = capi.Context(W, H, 10, max_frames=frames)
    plane = Plane(torch, [ds[f % 4]["pic"] for f in range(frames)])
    first, first4, fold, merge = (np.stack([ds[f % 4][key] for f in range(frames)]) for key in ("first", "first4", "fold", "merge"))
    assert first.shape[0] * first.shape[1] == 1044
    qp = 27
    exp4 = [nx.expected(d["pic"], 10, qp, d["first"], d["first4"], d["fold"], d["merge"], 3) for d in ds]
    got, gx = run(torch, ctx, plane, first, first4, qp, fold, merge, 3, in_place=True)
    for f in range(frames):
        assert got[f].tobytes() == exp4[f % 4][0].tobytes() and gx[f].tobytes() == exp4[f % 4][1].tobytes(), f
    ctx.close()


def test_two_streams_with_different_qps(torch_cuda):
    torch = torch_cuda
    d = nx.draw(4)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]])
    qps = (10, 37)
    exp = [nx.expected(d["pic"], d["bd"], qp, d["first"], d["first4"], d["fold"], d["merge"], 3) for qp in qps]
    assert exp[0][0].tobytes() != exp[1][0].tobytes()
    held, held4, held_f, held_m = (to_dev(torch, d[k]) for k in ("first", "first4", "fold", "merge"))
    streams = [torch.cuda.Stream() for _ in qps]
    outs = [[(Guarded(torch, N * 85 * 16), Guarded(torch, N * 64 * 16)) for _ in range(3)] for _ in qps]
    torch.cuda.synchronize()
    for r in range(3):
        for s, qp, o in zip(streams, qps, outs):
            ctx.intra_rd_nxn_device(plane.ptr, 2, plane.stride, 0, 1, held.data_ptr(), held4.data_ptr(), o[r][0].ptr, o[r][1].ptr, d_fold=held_f.data_ptr(),
                                    d_rd_merge=held_m.data_ptr(), skip_mask=3, stream=s.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    for e, o in zip(exp, outs):
        for r in range(3):
            nx.same(o[r][0].result(PDT, e[0].shape), e[0], r)
            nx.same(o[r][1].result(XDT, e[1].shape), e[1], r)
    ctx.close()


# ---- 4. chains ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, dtype", [(8, np.uint8), (10, np.int16), (12, np.int16)])
def test_both_first_passes_and_the_stage_on_one_stream(torch_cuda, bd, dtype):
    """4x4 first pass -> first pass -> stage on one stream without a host synchronisation, against the oracle's first passes and the restatement"""
    torch = torch_cuda
    qp = 27
    pic = ir.draw_picture(bd, 40)
    first, first4 = ir.first_pass(pic, bd, qp), nx.real_first4(pic, bd, qp)
    ep, ex = nx.plain(pic, bd, qp, first, first4)
    assert (ep["part"] == nx.PART_NXN).sum() > 20
    ctx = capi.Context(W, H, bd)
    plane = Plane(torch, [pic], dtype)
    d_first, d_first4, out, outx = Guarded(torch, N * 85 * 16), Guarded(torch, N * 256 * 16), Guarded(torch, N * 85 * 16), Guarded(torch, N * 64 * 16)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.intra_first_pass_4x4_device(plane.ptr, plane.item, plane.stride, 0, 1, d_first4.ptr, None, stream=stream.cuda_stream, qp=qp, num_candidates=0)
    ctx.intra_first_pass_device(plane.ptr, plane.item, plane.stride, 0, 1, d_first.ptr, stream=stream.cuda_stream, qp=qp)
    ctx.intra_rd_nxn_device(plane.ptr, plane.item, plane.stride, 0, 1, d_first.ptr, d_first4.ptr, out.ptr, outx.ptr, stream=stream.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    g4 = d_first4.result(NDT, (N, 256))
    assert np.array_equal(g4["satd"], first4["satd"]) and np.array_equal(g4["mode"], first4["mode"])
    nx.same(outx.result(XDT, (N, 64)), ex, bd)
    nx.same(out.result(PDT, (N, 85)), ep, bd)
    ctx.close()


@pytest.mark.parametrize("coarse_range", [0, 6])
def test_frame_against_its_pieces_and_its_counters(torch_cuda, coarse_range):
    """fhevc_p_tree_rd_intra_nxn_frame: fhevc_p_tree_rd_qt_frame's records at 3 taken as d_fold, the two first passes of the current picture, this stage
    in place, the RD tree -- through the host forms and on the device"""
    torch = torch_cuda
    bd, qp, mask = 8, 27, 3
    ref, cur = frame_pictures(bd)
    (bc, org, stride), (br, _, _) = pel(cur), pel(ref)
    ctx = capi.Context(W, H, bd)
    kw = dict(origin=org, stride=stride, qp=qp, search_range=8, coarse_range=coarse_range, skip_mask=mask)
    every = dict(with_shapes=True, with_merge=True, with_rd_merge=True, with_rd_pu=True)
    base = ctx.p_tree_rd_qt_frame(bc, br, 3, **every, **kw)
    s0 = ctx.stats()
    qt = ctx.p_tree_rd_intra_qt_frame(bc, br, 3, with_first=True, **every, **kw)
    s1 = ctx.stats()
    got = ctx.p_tree_rd_intra_nxn_frame(bc, br, with_first=True, with_nxn=True, **every, **kw)
    s2 = ctx.stats()
    first = ctx.intra_first_pass(bc, org, stride, qp=qp)
    first4, _ = ctx.intra_first_pass_4x4(bc, org, stride, qp=qp)
    assert len(got) == 8 and got[6].tobytes() == first.tobytes() and all(got[i].tobytes() == base[i].tobytes() for i in (2, 3, 4))
    folded, x = ctx.intra_rd_nxn(bc, first, first4, fold=base[5], rd_merge=base[4], skip_mask=mask, origin=org, stride=stride, qp=qp, with_nxn=True)
    ep, ex = nx.expected(cur, bd, qp, first, first4, base[5], base[4], mask)
    nx.same(folded, ep, "host form against the restatement")
    nx.same(x, ex, "host form's NxN records")
    assert got[5].tobytes() == folded.tobytes() and got[7].tobytes() == x.tobytes()
    unfolded, _ = nx.plain(cur, bd, qp, first, first4)
    assert (unfolded["part"] == nx.PART_NXN).sum() > 20 and (folded["part"] >= ir.PART_INTRA).any() and (folded["part"] < ir.PART_INTRA).any()
    print("NxN records that survive the fold:", int((folded["part"] == nx.PART_NXN).sum()), "; records that differ from the chain without the candidate:",
          int((folded.view(np.uint8).reshape(-1, 16) != qt[5].view(np.uint8).reshape(-1, 16)).any(axis=1).sum()))
    dev, dx = run(torch, ctx, Plane(torch, [cur]), first[None], first4[None], qp, base[5][None], base[4][None], mask, in_place=True)
    assert dev[0].tobytes() == folded.tobytes() and dx[0].tobytes() == x.tobytes()
    dmin, dmax = capi.p_tree_select_rd_pu(folded, base[4], mask, W, H)
    assert np.array_equal(got[0], dmin) and np.array_equal(got[1], dmax)
    # the counters: one launch more than the chain without the candidate (the 4x4 first pass), the same uploads, the NxN records down beside the rest
    assert (s2["kernels_launched"] - s1["kernels_launched"]) - (s1["kernels_launched"] - s0["kernels_launched"]) == 1
    assert s2["bytes_h2d"] - s1["bytes_h2d"] == s1["bytes_h2d"] - s0["bytes_h2d"]
    assert (s2["bytes_d2h"] - s1["bytes_d2h"]) - (s1["bytes_d2h"] - s0["bytes_d2h"]) == N * 64 * 16
    # without the NxN records asked for, the rest is the same
    less = ctx.p_tree_rd_intra_nxn_frame(bc, br, with_first=True, **every, **kw)
    assert len(less) == 7 and all(a.tobytes() == b.tobytes() for a, b in zip(less, got))
    ctx.close()


def test_host_form_equals_device_form_and_counts_what_it_moves(torch_cuda):
    torch = torch_cuda
    d = nx.draw(5)
    ctx = capi.Context(W, H, d["bd"])
    buf, org, stride = pel(d["pic"])
    for fold, merge, mask, with_nxn in ((None, None, 0, True), (d["fold"], None, 0, False), (d["fold"], d["merge"], 3, True), (None, d["merge"], 1, True)):
        before = ctx.stats()
        host = ctx.intra_rd_nxn(buf, d["first"], d["first4"], fold=fold, rd_merge=merge, skip_mask=mask, origin=org, stride=stride, qp=d["qp"], with_nxn=with_nxn)
        after = ctx.stats()
        dev, dx = run(torch, ctx, Plane(torch, [d["pic"]]), d["first"][None], d["first4"][None], d["qp"], None if fold is None else fold[None],
                      None if merge is None else merge[None], mask)
        hr, hx = host if with_nxn else (host, None)
        assert hr.tobytes() == dev[0].tobytes() and (hx is None or hx.tobytes() == dx[0].tobytes())
        nx.same(hr, ir.gate_fold(d["plain"], fold, merge, mask), "host form")
        arrays = 1 + (fold is not None) + (merge is not None)
        assert after["bytes_h2d"] - before["bytes_h2d"] == 2 * W * H + arrays * N * 85 * 16 + N * 256 * 16
        assert after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16 + (N * 64 * 16 if with_nxn else 0)
        assert after["kernels_launched"] - before["kernels_launched"] == 1
    none = ctx.intra_rd_nxn(buf, d["first"], None, fold=d["fold"], rd_merge=d["merge"], skip_mask=3, origin=org, stride=stride, qp=d["qp"])
    assert none.tobytes() == ctx.intra_rd_qt(buf, d["first"], 3, fold=d["fold"], rd_merge=d["merge"], skip_mask=3, origin=org, stride=stride, qp=d["qp"]).tobytes()
    ctx.close()


# ---- 5. rejected calls, the timing slot --------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing_and_the_timing_slot(torch_cuda):
    torch = torch_cuda
    d = nx.draw(1)
    ctx = capi.Context(W, H, 10, max_frames=2)
    plane = Plane(torch, [d["pic"], d["pic"]])
    first, first4, fold, merge = (to_dev(torch, np.stack([a, a])) for a in (d["first"], d["first4"], d["fold"], d["merge"]))
    extent, xextent, extent4 = 2 * N * 85 * 16, 2 * N * 64 * 16, 2 * N * 256 * 16
    out, outx = Guarded(torch, extent + 64), Guarded(torch, xextent + 64)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=plane.ptr, sb=2, stride=plane.stride, fs=plane.fstride, nf=2, rb=0, re=CH, qp=30, first=first.data_ptr(), first4=first4.data_ptr(),
                fold=fold.data_ptr(), merge=merge.data_ptr(), mask=3, out=out.ptr, nxn=outx.ptr)
    bad = [(dict(ctx=None), None), (dict(first4=None), "need"), (dict(luma=None), "argument"), (dict(first=None), "argument"), (dict(out=None), "argument"),
           (dict(nf=0), "layout"), (dict(sb=3), "layout"), (dict(stride=W - 1), "layout"), (dict(qp=-1), "qp"), (dict(qp=52), "qp"), (dict(rb=-1), "band"),
           (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"), (dict(sb=1), "uint8"), (dict(mask=-1), "skip_mask"), (dict(mask=4), "skip_mask"),
           (dict(first=first.data_ptr() + 2), "aligned"), (dict(first4=first4.data_ptr() + 2), "aligned"), (dict(first4=first4.data_ptr() + 1), "aligned"),
           (dict(fold=fold.data_ptr() + 2), "aligned"), (dict(merge=merge.data_ptr() + 1), "aligned"), (dict(out=out.ptr + 2), "aligned"), (dict(nxn=outx.ptr + 2), "aligned"),
           (dict(nxn=outx.ptr + 3), "aligned"), (dict(fold=out.ptr + 16), "overlaps"), (dict(fold=out.ptr - 16), "overlaps"),
           (dict(nxn=out.ptr), "overlap"), (dict(nxn=out.ptr + extent - 16), "overlap"), (dict(nxn=fold.data_ptr()), "overlap"), (dict(nxn=merge.data_ptr() + 32), "overlap"),
           (dict(nxn=first.data_ptr() + extent - 4), "overlap"), (dict(nxn=first4.data_ptr() - xextent + 4), "overlap"), (dict(nxn=first4.data_ptr() + extent4 - 4), "overlap"),
           (dict(nxn=plane.ptr), "overlap")]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_intra_rd_nxn_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["first"], a["first4"], a["fold"],
                                             a["merge"], a["mask"], a["out"], a["nxn"], None)
    for change, text in bad:
        assert call(dict(good, **change)) == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert out.untouched() and outx.untouched() and ctx.stats()["kernels_launched"] == launched
    # the host form and the frame call
    buf, org, stride = pel(d["pic"])
    res = np.full((N, 85), CANARY, np.uint8).repeat(16, axis=1).view(PDT)
    resx = np.full((N, 64), CANARY, np.uint8).repeat(16, axis=1).view(XDT)
    before = ctx.stats()
    for qp, mask, st, f4 in ((52, 3, stride, d["first4"].ctypes.data), (30, 4, stride, d["first4"].ctypes.data), (30, 3, W - 1, d["first4"].ctypes.data), (30, 3, stride, None)):
        assert lib.fhevc_intra_rd_nxn(ctx.h, buf.ctypes.data + 2 * org, st, qp, d["first"].ctypes.data, f4, None, None, mask, res.ctypes.data, resx.ctypes.data) == capi.E_INVALID
    maps = np.full((2, N * 256), CANARY, np.uint8)
    for qp, mask in ((52, 3), (30, 4), (30, -1)):
        assert lib.fhevc_p_tree_rd_intra_nxn_frame(ctx.h, buf.ctypes.data + 2 * org, buf.ctypes.data + 2 * org, stride, qp, 8, 0, None, None, mask, maps[0].ctypes.data,
                                                   maps[1].ctypes.data, None, None, None, res.ctypes.data, None, resx.ctypes.data) == capi.E_INVALID
    assert (res.view(np.uint8) == CANARY).all() and (resx.view(np.uint8) == CANARY).all() and (maps == CANARY).all() and ctx.stats() == before
    # slot 39 counts one launch per call; 17, 29, 31, 33, 35 and 37 stay untouched; 38 and 40 are no slots
    ctx.enable_kernel_timing(True)
    slots = (17, 29, 31, 33, 35, 37, 39)
    for s in slots:
        ctx.kernel_timing(s, reset=True)
    for _ in range(3):
        assert call(good) == capi.OK
    torch.cuda.synchronize()
    ms, n = ctx.kernel_timing(39)
    assert n == 3 and ms > 0.0 and all(ctx.kernel_timing(s)[1] == 0 for s in (17, 29, 31, 33, 35, 37))
    assert ctx.kernel_timing(39, reset=True)[1] == 3 and ctx.kernel_timing(39)[1] == 0
    for s in (38, 40):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()
