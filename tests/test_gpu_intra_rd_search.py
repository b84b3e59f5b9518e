"""Config 4 (P slices): the intra RD stage that searches the first pass's candidate lists (fhevc_intra_rd_search*: the two search instances of
k_motion_rd.hip) on the MI355X, byte for byte on BOTH outputs against the restatement tests/intra_rd_search_ref.py, which tests/test_intra_rd_search_ref.py
holds to intra_rd_qt_ref, intra_rd_nxn_ref and closed forms without a GPU.  Nothing is compared with the kernel's own output except where two launches must
give the same bytes.

The draw's pictures are 168 x 152 (3 x 3 CTUs, ragged on both sides); the other shapes are 64 x 64 and 72 x 72."""
import numpy as np
import pytest

import intra_rd_nxn_ref as nx
import intra_rd_qt_ref as iq
import intra_rd_ref as ir
import intra_rd_search_ref as sr
import motion_rd_ref as rd
from fasthevc_amd import capi
from motion_gpu_helpers import to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)
from test_gpu_intra_rd import Guarded, Plane, at_offset

pytestmark = pytest.mark.gpu

PDT, NDT, XDT = sr.PDT, sr.NDT, sr.XDT
W, H, N = ir.DRAW_W, ir.DRAW_H, ir.DRAW_N
FIRST_OF_DEPTH = {bd: next(i for i, e in enumerate(ir.DRAW) if e[0] == bd) for bd in (8, 10, 12)}


def run(torch, ctx, plane, modes, modes4, qp, rule=None, fold=None, merge=None, mask=0, rows=None, in_place=False, offs=(0, 0), out_off=0, offx=0, stream=None, with_nxn=True):
    """modes [F, band CTUs, 85, stride], modes4 [F, band CTUs, 256, stride4] or None -> (the records written [F, band CTUs, 85], the NxN records [F, band CTUs, 64]
    or None); both outputs lie between canaries (in place: the fold records lie in the first)"""
    held = at_offset(torch, modes, offs[0])
    held4 = at_offset(torch, modes4, offs[1]) if modes4 is not None else (None, None)
    held_m = at_offset(torch, merge, 0) if merge is not None else (None, None)
    shape = modes.shape[:3]
    count = int(np.prod(shape))
    out = Guarded(torch, count * 16, out_off)
    with_nxn = with_nxn and modes4 is not None
    outx = Guarded(torch, count // 85 * 64 * 16, offx) if with_nxn else None
    held_f = (None, None)
    if fold is not None and in_place:
        out.t[out.off:out.off + out.n] = to_dev(torch, fold)
        held_f = (None, out.ptr)
    elif fold is not None:
        held_f = at_offset(torch, fold, 0)
    torch.cuda.synchronize()
    ctx.intra_rd_search_device(plane.ptr, plane.item, plane.stride, plane.fstride, plane.frames, held[1], modes.shape[-1], held4[1], modes4.shape[-1] if modes4 is not None else 0,
                               out.ptr, rule=sr.rule_of(rule or sr.DEFAULT), d_nxn=outx.ptr if with_nxn else None, d_fold=held_f[1], d_rd_merge=held_m[1], skip_mask=mask, rows=rows,
                               stream=stream, qp=qp)
    torch.cuda.synchronize()
    return out.result(PDT, shape), outx.result(XDT, shape[:2] + (64,)) if with_nxn else None


# ---- 1. the draw, byte for byte ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, dtype", [(8, np.int16), (8, np.uint8), (10, np.int16), (12, np.int16)])
def test_the_draw_both_outputs_plain_and_every_combination_of_gate_and_fold(torch_cuda, bd, dtype):
    torch = torch_cuda
    ctx = capi.Context(W, H, bd)
    ctx.enable_kernel_timing(True)
    for s in (33, 37, 39, 41):
        ctx.kernel_timing(s, reset=True)
    d = sr.draw(FIRST_OF_DEPTH[bd])
    qp = d["qp"]
    plane = Plane(torch, [d["pic"]], dtype)
    modes, modes4 = d["modes"][None], d["modes4"][None]
    got, gx = run(torch, ctx, plane, modes, modes4, qp)
    sr.same(gx[0], d["nxn"], "nxn")
    sr.same(got[0], d["plain"], "plain")
    st = d["stats"]
    assert (st["pos"] > 0).sum() > 50 and st["second_won"].sum() > 8 and st["planar_won"].sum() > 8 and (got[0]["part"] == nx.PART_NXN).sum() > 8
    nox, none = run(torch, ctx, plane, modes, modes4, qp, with_nxn=False)
    assert none is None and nox.tobytes() == got.tobytes()
    calls = 2
    for fold in (None, "second", "in place"):
        for merge, masks in ((None, (0, 3)), (d["merge"], (0, 1, 2, 3))):
            for mask in masks:
                exp = ir.gate_fold(d["plain"], d["fold"] if fold else None, merge, mask)
                res, rx = run(torch, ctx, plane, modes, modes4, qp, fold=d["fold"][None] if fold else None, merge=None if merge is None else merge[None], mask=mask,
                              in_place=fold == "in place")
                calls += 1
                sr.same(res[0], exp, (fold, merge is not None, mask))
                assert rx.tobytes() == gx.tobytes()          # the NxN records do not depend on the gate, the fold or the choice
    # without the 4x4 lists there is no NxN candidate
    exp2, none = sr.expected(d["pic"], bd, qp, d["modes"], None, fold=d["fold"], rd_merge=d["merge"], skip_mask=3)
    got2, _ = run(torch, ctx, plane, modes, None, qp, fold=d["fold"][None], merge=d["merge"][None], mask=3)
    sr.same(got2[0], exp2, "no 4x4 lists")
    assert ctx.kernel_timing(41)[1] == calls + 1 and all(ctx.kernel_timing(s)[1] == 0 for s in (33, 37, 39))   # ONE launch per call, under slot 41 alone
    ctx.close()


@pytest.mark.parametrize("index", range(len(ir.DRAW)))
def test_the_whole_draw_both_outputs_plain_and_gated_and_folded_in_place(torch_cuda, index):
    """every picture of the draw (one in five on the oracle's own lists), uint8 planes for every other 8-bit picture"""
    torch = torch_cuda
    d = sr.draw(index)
    ctx = capi.Context(W, H, d["bd"])
    plane = Plane(torch, [d["pic"]], np.uint8 if d["bd"] == 8 and index % 2 else np.int16)
    got, gx = run(torch, ctx, plane, d["modes"][None], d["modes4"][None], d["qp"])
    sr.same(gx[0], d["nxn"], ("nxn", index))
    sr.same(got[0], d["plain"], ("plain", index))
    res, rx = run(torch, ctx, plane, d["modes"][None], d["modes4"][None], d["qp"], fold=d["fold"][None], merge=d["merge"][None], mask=3, in_place=True)
    sr.same(res[0], ir.gate_fold(d["plain"], d["fold"], d["merge"], 3), ("folded", index))
    assert rx.tobytes() == gx.tobytes()
    ctx.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_both_first_passes_then_the_stage_on_one_stream(torch_cuda, bd):
    """the lists never leave the device and nothing waits between the three launches"""
    torch = torch_cuda
    from motion_gpu_helpers import pel
    d = sr.draw([i for i, e in enumerate(ir.DRAW) if e[0] == bd][1])
    qp = d["qp"]
    ctx = capi.Context(W, H, bd)
    plane = Plane(torch, [d["pic"]])
    lists, lists4 = Guarded(torch, N * 85 * 8), Guarded(torch, N * 256 * 8)
    out, outx = Guarded(torch, N * 85 * 16), Guarded(torch, N * 64 * 16)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.intra_first_pass_candidates_device(plane.ptr, plane.item, plane.stride, 0, 1, lists.ptr, stream=stream.cuda_stream, qp=qp, num_candidates=8)
    ctx.intra_first_pass_4x4_device(plane.ptr, plane.item, plane.stride, 0, 1, None, lists4.ptr, stream=stream.cuda_stream, qp=qp, num_candidates=8)
    ctx.intra_rd_search_device(plane.ptr, plane.item, plane.stride, 0, 1, lists.ptr, 8, lists4.ptr, 8, out.ptr, d_nxn=outx.ptr, stream=stream.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    buf, org, stride = pel(d["pic"])
    modes = ctx.intra_first_pass_candidates(buf, org, stride, qp=qp, num_candidates=8)
    _, modes4 = ctx.intra_first_pass_4x4(buf, org, stride, qp=qp, num_candidates=8)
    assert lists.result(np.uint8, (N, 85, 8)).tobytes() == modes.tobytes() and lists4.result(np.uint8, (N, 256, 8)).tobytes() == modes4.tobytes()
    ep, ex = sr.plain(d["pic"], bd, qp, modes, modes4)
    sr.same(out.result(PDT, (N, 85)), ep, bd)
    sr.same(outx.result(XDT, (N, 64)), ex, bd)
    ctx.close()


# ---- 2. the identities on the device ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10])
def test_identity_i_against_the_nxn_stage_and_identity_ii_against_the_three_depth_stage(torch_cuda, bd):
    torch = torch_cuda
    d = sr.draw(FIRST_OF_DEPTH[bd])
    qp = d["qp"]
    ctx = capi.Context(W, H, bd)
    plane = Plane(torch, [d["pic"]])
    one = dict(count=(1, 1, 1, 1), count4=1, append_planar=0)
    first, first4 = sr.first_of(d["modes"]), sr.first_of(d["modes4"])
    for with4 in (True, False):
        got, gx = run(torch, ctx, plane, d["modes"][None], d["modes4"][None] if with4 else None, qp, rule=one, fold=d["fold"][None], merge=d["merge"][None], mask=3)
        out, outx = Guarded(torch, N * 85 * 16), Guarded(torch, N * 64 * 16)
        hf, h4, hfo, hm = to_dev(torch, first), to_dev(torch, first4), to_dev(torch, d["fold"]), to_dev(torch, d["merge"])
        torch.cuda.synchronize()
        ctx.intra_rd_nxn_device(plane.ptr, 2, plane.stride, 0, 1, hf.data_ptr(), h4.data_ptr() if with4 else None, out.ptr, outx.ptr if with4 else None, d_fold=hfo.data_ptr(),
                                d_rd_merge=hm.data_ptr(), skip_mask=3, qp=qp)
        torch.cuda.synchronize()
        assert out.result(PDT, (N, 85)).tobytes() == got[0].tobytes()          # pad[1] is 0 on both sides
        if with4:
            assert outx.result(XDT, (N, 64)).tobytes() == gx[0].tobytes()
    # (ii): any node's record is the three-depth stage's for the winning mode, in all bytes but pad[1]
    got, _ = run(torch, ctx, plane, d["modes"][None], None, qp)
    win = np.zeros((N, 85), NDT)
    win["mode"] = np.where(got[0]["part"] == 255, 255, got[0]["pad"][..., 0])
    out = Guarded(torch, N * 85 * 16)
    hw = to_dev(torch, win)
    torch.cuda.synchronize()
    ctx.intra_rd_qt_device(plane.ptr, 2, plane.stride, 0, 1, hw.data_ptr(), 3, out.ptr, qp=qp)
    torch.cuda.synchronize()
    same = got[0].copy()
    same["pad"][..., 1] = 0
    assert out.result(PDT, (N, 85)).tobytes() == same.tobytes()
    ctx.close()


# ---- 3. other rules and strides; shapes; bands; list pointers at every byte offset ------------------------------------------------------------------------

@pytest.mark.parametrize("rule, stride, stride4", [(dict(count=(1, 2, 3, 8), count4=8, append_planar=1), 8, 8), (dict(count=(3, 3, 3, 3), count4=1, append_planar=0), 3, 3),
                                                   (dict(count=(2, 3, 1, 3), count4=3, append_planar=1), 3, 8)])
def test_other_rules_and_strides_on_the_ragged_picture_at_every_byte_offset(torch_cuda, rule, stride, stride4):
    torch = torch_cuda
    bd, qp = 10, 30
    rng = np.random.default_rng(stride * 10 + stride4)
    pic = rng.integers(0, 1 << bd, size=(72, 72)).astype(np.int16)
    pic[:, 20:60] = (pic[:, 20:60] >> 3) + 300          # a calmer middle, so that not every mode costs the same
    modes, modes4 = sr.random_lists(rng, 4, 85)[..., :stride].copy(), sr.random_lists(rng, 4, 256)[..., :stride4].copy()
    exp, ex = sr.expected(pic, bd, qp, modes, modes4, rule)
    ctx = capi.Context(72, 72, bd)
    plane = Plane(torch, [pic])
    for off in range(4):
        got, gx = run(torch, ctx, plane, modes[None], modes4[None], qp, rule=rule, offs=(off, 3 - off), out_off=(0, 4, 8, 12)[off], offx=(12, 8, 4, 0)[off])
        sr.same(got[0], exp, ("out", off))
        sr.same(gx[0], ex, ("nxn", off))
    # bands are slices; the empty band writes nothing
    for rows in ((0, 1), (1, 2)):
        sl = slice(rows[0] * 2, rows[1] * 2)
        got, gx = run(torch, ctx, plane, modes[None, sl], modes4[None, sl], qp, rule=rule, rows=rows)
        sr.same(got[0], exp[sl], rows)
        sr.same(gx[0], ex[sl], rows)
    ctx.close()


def test_the_constant_picture_and_the_stripe_picture_with_the_right_modes_last(torch_cuda):
    torch = torch_cuda
    for bd, qp in ((8, 27), (10, 32)):
        lam = rd.lam_q8(qp)
        ctx = capi.Context(64, 64, bd)
        flat = iq.constant_picture(64, 64, bd, 1 << (bd - 1))
        rng = np.random.default_rng(bd)
        modes, modes4 = rng.integers(1, 35, size=(1, 1, 85, 8)).astype(np.uint8), rng.integers(1, 35, size=(1, 1, 256, 8)).astype(np.uint8)
        got, gx = run(torch, ctx, Plane(torch, [flat]), modes, modes4, qp)
        # every mode predicts a constant picture exactly: the appended planar, the cheapest flag, wins everywhere -- section 4.16's numbers with planar
        assert (got[0, 0]["part"] == ir.PART_INTRA).all() and (got[0, 0]["pad"][1:, 0] == 0).all() and (got[0, 0]["dist"] == 0).all()
        assert (got[0, 0, 21:]["cost_rd"] == (4 * lam) >> 8).all() and (got[0, 0, 21:]["pad"][:, 1] == 8).all() and (got[0, 0, 1:21]["pad"][:, 1] == 3).all()
        assert (gx["dist"] == 0).all() and (gx["bits"] == 12).all() and (gx["cost_rd"] == (12 * lam) >> 8).all() and (gx["modes"] == 0).all()
        pic = nx.quadrant_stripes(64, 64, bd, 8, 8)
        m4 = np.full((1, 1, 256, 8), 1, np.uint8)
        m4[0, 0, nx.units(9), 7] = nx.STRIPE_MODES
        rule = dict(count=(3, 3, 3, 8), count4=8, append_planar=0)
        got, gx = run(torch, ctx, Plane(torch, [pic]), modes, m4, qp, rule=rule)
        assert gx[0, 0, 9]["dist"] == 0 and tuple(gx[0, 0, 9]["modes"]) == nx.STRIPE_MODES
        exp, ex = sr.expected(pic, bd, qp, modes[0], m4[0], rule)
        sr.same(got[0], exp, "stripes")
        sr.same(gx[0], ex, "stripes nxn")
        ctx.close()


# ---- 4. poisoned planes; a thousand CTUs in one launch; two streams; the host form; rejected calls ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.int16, np.uint8])
def test_poisoned_planes_with_odd_origin_and_stride(torch_cuda, dtype):
    """the picture inside a plane of random samples, its origin and stride odd: nothing outside the picture is read for its value, and the per-sample staging
    path of the search instances gives the bytes of the 16-byte one -- both outputs"""
    torch = torch_cuda
    d = sr.draw(6 if dtype == np.uint8 else 4)
    bd = d["bd"]
    assert bd == (8 if dtype == np.uint8 else 10)
    ctx = capi.Context(W, H, bd)
    item = np.dtype(dtype).itemsize
    hm, h4 = to_dev(torch, d["modes"]), to_dev(torch, d["modes4"])
    for seed, (stride, org) in enumerate(((W + 13, 3 * (W + 13) + 5), (W + 1, W + 1 + 1), (W, 7))):
        rng = np.random.default_rng(seed)
        buf = rng.integers(0, 1 << bd, size=org + H * stride + 64).astype(dtype)
        for y in range(H):
            buf[org + y * stride:org + y * stride + W] = d["pic"][y]
        t = to_dev(torch, buf)
        out, outx = Guarded(torch, N * 85 * 16), Guarded(torch, N * 64 * 16)
        torch.cuda.synchronize()
        ctx.intra_rd_search_device(t.data_ptr() + item * org, item, stride, 0, 1, hm.data_ptr(), 8, h4.data_ptr(), 8, out.ptr, d_nxn=outx.ptr, qp=d["qp"])
        torch.cuda.synchronize()
        sr.same(out.result(PDT, (N, 85)), d["plain"], (stride, org))
        sr.same(outx.result(XDT, (N, 64)), d["nxn"], (stride, org))
    ctx.close()


def test_a_thousand_ctus_in_one_launch(torch_cuda):
    torch = torch_cuda
    d = sr.draw(FIRST_OF_DEPTH[8])
    frames = 112                                          # 112 x 9 = 1 008 CTUs: more than the resident grid
    ctx = capi.Context(W, H, 8)
    plane = Plane(torch, [d["pic"]] * frames, np.uint8)
    modes, modes4 = np.repeat(d["modes"][None], frames, 0), np.repeat(d["modes4"][None], frames, 0)
    got, gx = run(torch, ctx, plane, modes, modes4, d["qp"])
    for f in (0, 57, frames - 1):
        sr.same(got[f], d["plain"], f)
        sr.same(gx[f], d["nxn"], f)
    assert all(got[f].tobytes() == got[0].tobytes() and gx[f].tobytes() == gx[0].tobytes() for f in range(frames))
    ctx.close()


def test_two_streams_with_different_qps_and_rules(torch_cuda):
    torch = torch_cuda
    d = sr.draw(FIRST_OF_DEPTH[8])
    other = dict(count=(1, 2, 3, 8), count4=2, append_planar=0)
    exp_b, ex_b = sr.plain(d["pic"], 8, 37, d["modes"], d["modes4"], other)
    ctx = capi.Context(W, H, 8)
    plane = Plane(torch, [d["pic"]])
    hm, h4 = to_dev(torch, d["modes"]), to_dev(torch, d["modes4"])
    outs = [(Guarded(torch, N * 85 * 16), Guarded(torch, N * 64 * 16)) for _ in range(2)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for (o, x), s, qp, rule in ((outs[0], s1, d["qp"], sr.DEFAULT), (outs[1], s2, 37, other)):
        ctx.intra_rd_search_device(plane.ptr, 2, plane.stride, 0, 1, hm.data_ptr(), 8, h4.data_ptr(), 8, o.ptr, rule=sr.rule_of(rule), d_nxn=x.ptr, stream=s.cuda_stream, qp=qp)
    torch.cuda.synchronize()
    sr.same(outs[0][0].result(PDT, (N, 85)), d["plain"], "stream 1")
    sr.same(outs[0][1].result(XDT, (N, 64)), d["nxn"], "stream 1")
    sr.same(outs[1][0].result(PDT, (N, 85)), exp_b, "stream 2")
    sr.same(outs[1][1].result(XDT, (N, 64)), ex_b, "stream 2")
    ctx.close()


def test_the_host_form_is_the_device_form_with_its_counters(torch_cuda):
    d = sr.draw(FIRST_OF_DEPTH[10])
    ctx = capi.Context(W, H, 10)
    exp = ir.gate_fold(d["plain"], d["fold"], d["merge"], 3)
    before = ctx.stats()
    got, gx = ctx.intra_rd_search(d["pic"].astype(np.int16), d["modes"], d["modes4"], fold=d["fold"], rd_merge=d["merge"], skip_mask=3, qp=d["qp"], with_nxn=True)
    after = ctx.stats()
    sr.same(got, exp, "host form")
    sr.same(gx, d["nxn"], "host form nxn")
    up = W * H * 2 + N * 85 * 8 + N * 256 * 8 + 2 * N * 85 * 16
    assert after["bytes_h2d"] - before["bytes_h2d"] == up and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16 + N * 64 * 16
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    dev, dx = run(torch_cuda, ctx, Plane(torch_cuda, [d["pic"]]), d["modes"][None], d["modes4"][None], d["qp"], fold=d["fold"][None], merge=d["merge"][None], mask=3)
    assert dev[0].tobytes() == got.tobytes() and dx[0].tobytes() == gx.tobytes()          # host form against device form
    # without the optional arrays: the lists alone go up, the records alone come down
    before = ctx.stats()
    less = ctx.intra_rd_search(d["pic"].astype(np.int16), d["modes"], None, qp=d["qp"])
    after = ctx.stats()
    dev2, _ = run(torch_cuda, ctx, Plane(torch_cuda, [d["pic"]]), d["modes"][None], None, d["qp"])
    assert dev2[0].tobytes() == less.tobytes()
    assert after["bytes_h2d"] - before["bytes_h2d"] == W * H * 2 + N * 85 * 8 and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    ctx.close()


def test_every_rejected_call_writes_nothing_and_launches_nothing(torch_cuda):
    torch = torch_cuda
    d = sr.draw(FIRST_OF_DEPTH[8])
    ctx = capi.Context(W, H, 8)
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(41, reset=True)
    plane = Plane(torch, [d["pic"]])
    hm, h4 = to_dev(torch, d["modes"]), to_dev(torch, d["modes4"])
    out, outx = Guarded(torch, N * 85 * 16), Guarded(torch, N * 64 * 16)
    torch.cuda.synchronize()

    def call(modes=hm.data_ptr(), stride=8, modes4=h4.data_ptr(), stride4=8, rule=sr.DEFAULT, o=out.ptr, x=outx.ptr, mask=0, pad=0, rows=None, qp=30):
        r = sr.rule_of(rule)
        r.pad[1] = pad
        ctx.intra_rd_search_device(plane.ptr, 2, plane.stride, 0, 1, modes, stride, modes4, stride4, o, rule=r, d_nxn=x, skip_mask=mask, rows=rows, qp=qp)

    bad = [dict(modes=None), dict(stride=0), dict(stride=9), dict(stride4=0), dict(stride4=9), dict(rule=dict(count=(0, 3, 3, 8), count4=8, append_planar=1)),
           dict(rule=dict(count=(3, 3, 3, 8), count4=8, append_planar=1), stride=7), dict(rule=dict(count=(3, 3, 3, 8), count4=0, append_planar=1)),
           dict(rule=dict(count=(3, 3, 3, 8), count4=8, append_planar=1), stride4=7), dict(rule=dict(count=(3, 3, 3, 8), count4=8, append_planar=2)), dict(pad=1),
           dict(modes4=None), dict(mask=4), dict(qp=52), dict(o=None), dict(o=out.ptr + 2), dict(x=outx.ptr + 2), dict(modes=out.ptr + 16), dict(modes4=outx.ptr),
           dict(modes4=out.ptr), dict(x=out.ptr + 160), dict(rows=(2, 1)), dict(modes=outx.ptr + 64)]
    for kw in bad:
        with pytest.raises(capi.FastHevcError):
            call(**kw)
    # a NULL rule, which the wrapper never passes
    assert ctx.lib.fhevc_intra_rd_search_device(ctx.h, plane.ptr, 2, plane.stride, 0, 1, 0, 3, 30, hm.data_ptr(), 8, h4.data_ptr(), 8, None, None, None, 0, out.ptr, outx.ptr,
                                                None) == capi.E_INVALID
    call(rows=(1, 1))   # the empty band: accepted, nothing launched
    torch.cuda.synchronize()
    assert ctx.kernel_timing(41)[1] == 0
    assert out.untouched() and outx.untouched()
    call()
    torch.cuda.synchronize()
    assert ctx.kernel_timing(41)[1] == 1
    for s in (40, 42):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()


# ---- 5. the frame call against its pieces ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coarse_range", [0, 6])
def test_frame_against_its_pieces_and_its_counters(torch_cuda, coarse_range):
    """fhevc_p_tree_rd_intra_search_frame: fhevc_p_tree_rd_qt_frame's records at 3 taken as d_fold, both first passes' lists of the current picture (the
    library's own: real lists), this stage in place, the RD tree"""
    from motion_gpu_helpers import pel
    from test_gpu_intra_rd_qt import frame_pictures
    bd, qp, mask = 8, 27, 3
    ref, cur = frame_pictures(bd)
    (bc, org, stride), (br, _, _) = pel(cur), pel(ref)
    ctx = capi.Context(W, H, bd)
    kw = dict(origin=org, stride=stride, qp=qp, search_range=8, coarse_range=coarse_range, skip_mask=mask)
    every = dict(with_shapes=True, with_merge=True, with_rd_merge=True, with_rd_pu=True)
    base = ctx.p_tree_rd_qt_frame(bc, br, 3, **every, **kw)
    s0 = ctx.stats()
    nxn = ctx.p_tree_rd_intra_nxn_frame(bc, br, with_first=True, with_nxn=True, **every, **kw)
    s1 = ctx.stats()
    got = ctx.p_tree_rd_intra_search_frame(bc, br, with_first=True, with_nxn=True, **every, **kw)
    s2 = ctx.stats()
    first = ctx.intra_first_pass(bc, org, stride, qp=qp)
    modes = ctx.intra_first_pass_candidates(bc, org, stride, qp=qp, num_candidates=8)
    _, modes4 = ctx.intra_first_pass_4x4(bc, org, stride, qp=qp, num_candidates=8)
    assert len(got) == 8 and got[6].tobytes() == first.tobytes() and all(got[i].tobytes() == base[i].tobytes() for i in (2, 3, 4))
    ep, ex = sr.expected(cur, bd, qp, modes, modes4, sr.DEFAULT, base[5], base[4], mask)
    sr.same(got[5], ep, "the folded records against the restatement on the library's own lists")
    sr.same(got[7], ex, "the NxN records")
    dmin, dmax = capi.p_tree_select_rd_pu(got[5], base[4], mask, W, H)
    assert np.array_equal(got[0], dmin) and np.array_equal(got[1], dmax)
    # the counters: one launch more than the NxN chain (the node lists' pass), the same uploads and downloads
    assert (s2["kernels_launched"] - s1["kernels_launched"]) - (s1["kernels_launched"] - s0["kernels_launched"]) == 1
    assert s2["bytes_h2d"] - s1["bytes_h2d"] == s1["bytes_h2d"] - s0["bytes_h2d"] and s2["bytes_d2h"] - s1["bytes_d2h"] == s1["bytes_d2h"] - s0["bytes_d2h"]
    # another rule; and a bad one is rejected
    rule = dict(count=(1, 2, 3, 8), count4=4, append_planar=0)
    other = ctx.p_tree_rd_intra_search_frame(bc, br, rule=sr.rule_of(rule), with_rd_pu=True, **kw)
    sr.same(other[2], sr.expected(cur, bd, qp, modes, modes4, rule, base[5], base[4], mask)[0], "another rule")
    with pytest.raises(capi.FastHevcError):
        ctx.p_tree_rd_intra_search_frame(bc, br, rule=sr.rule_of(dict(count=(0, 2, 3, 8), count4=4, append_planar=0)), **kw)
    ctx.close()
