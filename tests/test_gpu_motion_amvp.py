"""Config 4 (P slices): the re-pricing of refined costs against neighbour predictors (k_motion_amvp.hip) and fhevc_p_tree_amvp_frame on the MI355X, byte for
byte against the Python restatement tests/motion_amvp_ref.py (pinned without a GPU by tests/test_motion_amvp_ref.py) and against the host twin
fhevc_motion_amvp_picture.  Nothing is compared with the kernel's own output except where two launches must give the same bytes.

The picture is 168 x 152 = 3 x 3 CTUs with a column 40 wide, a row 24 tall and the corner: the smallest picture in which a 64x64 node has a left, an
above and a diagonal neighbour.  The stage reads no samples, so a batch of picture pairs is a batch of record arrays: the draws of the restatement module
are the pairs of one launch, and their expected records are computed once for the whole file."""
import numpy as np
import pytest

import motion_amvp_ref as ar
import motion_merge_cases as mc
import motion_merge_pu_ref as mpr
import pu_shape_ref as sr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, clip_planes, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu


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

W, H = ar.DRAW_W, ar.DRAW_H
CW, CH, N = 3, 3, 9
FAMILIES = ("nodes", "pu", "small")
QDT, VDT, MDT, SDT = ar.QDT, ar.VDT, capi.MOTION_MERGE_DTYPE, capi.SHAPE_DTYPE
ALL = frozenset(FAMILIES)


def run(torch, ctx, ins, want_out=ALL, want_mvp=ALL, rows=None, stream=None, qp=ar.DRAW_QP, in_offset=0, out_offset=0, mvp_offset=0):
    """ins {family: [pairs, band CTUs, per]} (a family may be missing) -> ({family: records}, {family: predictor records}) of the outputs asked for; every
    output between canaries; the offsets put the arrays that many bytes behind a 16-byte boundary"""
    P, nb = ins["nodes"].shape[:2]
    held = {f: at_offset(torch, a, in_offset) for f, a in ins.items()}
    outs = {f: Guarded(torch, P * nb * ar.PER[f] * 16, out_offset) for f in want_out}
    mvps = {f: Guarded(torch, P * nb * ar.PER[f] * 8, mvp_offset) for f in want_mvp}
    torch.cuda.synchronize()
    ptr = lambda d, f: d[f].ptr if f in d else None
    ctx.motion_amvp_device(P + 1, held["nodes"][1], held["pu"][1] if "pu" in held else None, held["small"][1] if "small" in held else None,
                           *[ptr(outs, f) for f in FAMILIES], *[ptr(mvps, f) for f in FAMILIES], rows=rows, stream=stream, qp=qp)
    torch.cuda.synchronize()
    return ({f: g.result(QDT, (P, nb, ar.PER[f])) for f, g in outs.items()}, {f: g.result(VDT, (P, nb, ar.PER[f])) for f, g in mvps.items()})


def check(got, exp, what, sel=slice(None)):
    for j in (0, 1):
        for f, a in got[j].items():
            ar.same(a, exp[f][j][sel], (what, f, j))


@pytest.fixture(scope="module")
def ctxs(torch_cuda):
    c = {bd: capi.Context(W, H, bd, max_frames=2) for bd in (8, 10, 12)}
    yield c
    for x in c.values():
        x.close()


# ---- 1. the draw: byte for byte against the restatement and the host twin ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_draw_all_families_with_and_without_predictor_records(torch_cuda, ctxs, bd):
    ins, exp, _ = ar.draw_batch()
    got = run(torch_cuda, ctxs[bd], ins)
    check(got, exp, ("all", bd))
    # markers in, markers out; a CU that is not INSIDE gets the refinement's marker whatever the input holds
    for f in FAMILIES:
        no_price = got[1][f]["idx"] == 255
        assert no_price.any() and (got[0][f]["cost_best"][no_price] == ar.MARK).all() and (got[0][f]["cost_best"][~no_price] != ar.MARK).all()
    check(run(torch_cuda, ctxs[bd], ins, want_mvp=frozenset()), exp, ("records only", bd))
    check(run(torch_cuda, ctxs[bd], ins, want_out=frozenset()), exp, ("predictor records only", bd))
    # the host twin on the same arrays
    for d in (0, ar.DRAWS - 1):
        host = capi.motion_amvp_picture(ins["nodes"][d], ins["pu"][d], ins["small"][d], W, H, bit_depth=bd, qp=ar.DRAW_QP, with_mvp=True)
        for i, f in enumerate(FAMILIES):
            assert host[i].tobytes() == got[0][f][d].tobytes() and host[3 + i].tobytes() == got[1][f][d].tobytes(), (bd, d, f)


def test_each_family_alone_and_in_pairs(torch_cuda, ctxs):
    ins, exp, _ = ar.draw_batch()
    few = {f: a[:6] for f, a in ins.items()}
    for fams in (("nodes",), ("pu",), ("small",), ("nodes", "pu"), ("nodes", "small"), ("pu", "small")):
        given = {f: few[f] for f in set(fams) | {"nodes"}}                     # the nodes are always an input: neighbour vectors come from them
        check(run(torch_cuda, ctxs[8], given, want_out=frozenset(fams), want_mvp=frozenset(fams)), exp, fams, slice(0, 6))
        check(run(torch_cuda, ctxs[8], given, want_out=frozenset(fams[:1]), want_mvp=frozenset(fams[1:])), exp, (fams, "mixed"), slice(0, 6))
        check(run(torch_cuda, ctxs[8], few, want_out=frozenset(fams), want_mvp=frozenset()), exp, (fams, "inputs without outputs"), slice(0, 6))


# ---- 2. bands, guards, alignments, grid ----------------------------------------------------------------------------------------------------------------------

def test_bands_as_slices_and_the_empty_band(torch_cuda, ctxs):
    ins, _, _ = ar.draw_batch()
    ctx = ctxs[10]
    for rows in ((0, 1), (1, 2), (1, 3), (2, 3), (0, 2)):
        cut = {f: np.ascontiguousarray(a[:3, rows[0] * CW:rows[1] * CW]) for f, a in ins.items()}
        exp = [ar.expected_all(W, H, cut["nodes"][d], cut["pu"][d], cut["small"][d], 27, rows=rows) for d in range(3)]
        got = run(torch_cuda, ctx, cut, rows=rows, qp=27)
        for j in (0, 1):
            for f in FAMILIES:
                ar.same(got[j][f], np.stack([e[f][j] for e in exp]), (rows, f, j))
    # the empty band launches nothing and writes nothing
    launched = ctx.stats()["kernels_launched"]
    held = at_offset(torch_cuda, ins["nodes"][:1], 0)
    out = Guarded(torch_cuda, 4096)
    ctx.motion_amvp_device(2, held[1], d_out_nodes=out.ptr, rows=(2, 2))
    torch_cuda.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_pointers_off_16(torch_cuda, ctxs, offset):
    """inputs, outputs and predictor records 4, 8, 12 bytes behind a 16-byte boundary, one kind at a time and all together: the same bytes"""
    ins, exp, _ = ar.draw_batch()
    few = {f: a[:4] for f, a in ins.items()}
    for kw in (dict(in_offset=offset), dict(out_offset=offset), dict(mvp_offset=offset), dict(in_offset=offset, out_offset=16 - offset, mvp_offset=offset)):
        check(run(torch_cuda, ctxs[8], few, **kw), exp, kw, slice(0, 4))


def test_more_ctus_than_the_grid(torch_cuda, ctxs):
    """5 x 60 pairs of 9 CTUs: 2 700 workgroups' worth of work on a grid of at most 8 per CU"""
    ins, exp, _ = ar.draw_batch()
    props = torch_cuda.cuda.get_device_properties(0)
    reps = 5
    assert reps * ar.DRAWS * N > 8 * props.multi_processor_count
    tiled = {f: np.concatenate([a] * reps) for f, a in ins.items()}
    got = run(torch_cuda, ctxs[8], tiled)
    for j in (0, 1):
        for f in FAMILIES:
            ar.same(got[j][f], np.concatenate([exp[f][j]] * reps), ("tiled", f, j))


def test_two_streams_with_different_qps(torch_cuda, ctxs):
    torch = torch_cuda
    ins, _, _ = ar.draw_batch()
    ctx = ctxs[8]
    qps = (4, 51)
    parts = [{f: np.ascontiguousarray(a[i * 3:i * 3 + 3]) for f, a in ins.items()} for i in range(2)]
    exps = [[ar.expected_all(W, H, p["nodes"][d], p["pu"][d], p["small"][d], qp) for d in range(3)] for p, qp in zip(parts, qps)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    held = [{f: at_offset(torch, a, 0) for f, a in p.items()} for p in parts]
    outs = [{f: Guarded(torch, 3 * N * ar.PER[f] * 16) for f in FAMILIES} for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):                                                          # several launches per stream in flight
        for i in range(2):
            ctx.motion_amvp_device(4, held[i]["nodes"][1], held[i]["pu"][1], held[i]["small"][1], *[outs[i][f].ptr for f in FAMILIES], stream=streams[i].cuda_stream,
                                   qp=qps[i])
    torch.cuda.synchronize()
    for i in range(2):
        for f in FAMILIES:
            ar.same(outs[i][f].result(QDT, (3, N, ar.PER[f])), np.stack([e[f][0] for e in exps[i]]), (qps[i], f))
    assert (exps[0][0]["small"][0]["cost_best"] != exps[1][0]["small"][0]["cost_best"]).any()


# ---- 3. the real chain on one stream ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10])
def test_search_refinement_repricing_merge_selection_on_one_stream(oracle, torch_cuda, ctxs, bd):
    torch = torch_cuda
    qp, R = {8: 27, 10: 32}[bd], 8
    pics = clip_planes(frames.pan_clip(W, H, 2, seed=41 + bd, v_structure=-5, v_noise=3), bd, low_bits_seed=5)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=np.int16, poison=None)
    ctx = ctxs[bd]
    d_luma = to_dev(torch, flat)
    p = d_luma.data_ptr() + 2 * origin
    per = (85, 124, 384)
    found, fine, priced = ([Guarded(torch, N * k * 16) for k in per] for _ in range(3))
    mpu = [Guarded(torch, N * k * 16) for k in per[1:]]
    shapes = Guarded(torch, N * 85 * 16)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = st.cuda_stream
    ctx.motion_search_pu_wide_device(p, 2, stride, fstride, 2, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
    ctx.motion_refine_pu_wide_device(p, 2, stride, fstride, 2, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s, qp=qp, max_range=R)
    ctx.motion_amvp_device(2, fine[0].ptr, fine[1].ptr, fine[2].ptr, priced[0].ptr, priced[1].ptr, priced[2].ptr, stream=s, qp=qp)
    ctx.motion_merge_pu_device(p, 2, stride, fstride, 2, priced[0].ptr, mpu[0].ptr, mpu[1].ptr, stream=s, qp=qp, max_range=R)
    ctx.pu_shape_select_merge_device(priced[0].ptr, priced[1].ptr, priced[2].ptr, mpu[0].ptr, mpu[1].ptr, 1, shapes.ptr, stream=s)
    torch.cuda.synchronize()
    refined = [g.result(QDT, (N, k)) for g, k in zip(fine, per)]
    got = [g.result(QDT, (N, k)) for g, k in zip(priced, per)]
    exp = ar.expected_all(W, H, *refined, qp)
    cheaper = 0
    for f, r, g in zip(FAMILIES, refined, got):
        ar.same(g, exp[f][0], (bd, f))
        # the vectors and distortions are the refinement's: only the price changes
        for name in ("satd_int", "satd_best", "mvx", "mvy"):
            assert np.array_equal(g[name], r[name]), (f, name)
        ok = r["cost_best"] != ar.MARK
        assert ok.any() and np.array_equal(ok, g["cost_best"] != ar.MARK)
        cheaper += int((g["cost_best"][ok] < r["cost_best"][ok]).sum())
    assert cheaper > 0                                                          # a pan: entries have neighbours that move alike
    # the stages behind it consumed the re-priced records: the merge records rest on the vectors alone, the selection on the new costs
    emp = [mpu[i].result(MDT, (N, k)) for i, k in enumerate(per[1:])]
    erec = mpr.select(got[0][None], got[1][None], got[2][None], emp[0][None], emp[1][None], W, H)[0]
    sr.same(shapes.result(SDT, (N, 85)), erec[0], ("selection", bd))


# ---- 4. the host form and the frame chain -------------------------------------------------------------------------------------------------------------------

def test_host_form_equals_device_form_with_counters(torch_cuda, ctxs):
    ins, exp, _ = ar.draw_batch()
    ctx = ctxs[12]
    d = 5
    before = ctx.stats()
    got = ctx.motion_amvp(ins["nodes"][d], ins["pu"][d], ins["small"][d], qp=ar.DRAW_QP, with_mvp=True)
    after = ctx.stats()
    for i, f in enumerate(FAMILIES):
        ar.same(got[i], exp[f][0][d], ("host form", f))
        ar.same(got[3 + i], exp[f][1][d], ("host form mvp", f))
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    assert after["bytes_h2d"] - before["bytes_h2d"] == N * 593 * 16 and after["bytes_d2h"] - before["bytes_d2h"] == N * 593 * 24
    before = after
    (small,) = ctx.motion_amvp(ins["nodes"][d], None, ins["small"][d], qp=ar.DRAW_QP)[2:]
    ar.same(small, exp["small"][0][d], "host form, small alone")
    (nodes_mvp,) = ctx.motion_amvp(ins["nodes"][d], qp=ar.DRAW_QP, with_records=False, with_mvp=True)[:1]
    ar.same(nodes_mvp, exp["nodes"][1][d], "host form, predictor records of the nodes alone")
    after = ctx.stats()
    assert after["bytes_h2d"] - before["bytes_h2d"] == N * (2 * 85 + 384) * 16 and after["bytes_d2h"] - before["bytes_d2h"] == N * (384 * 16 + 85 * 8 + 85 * 16)
    with pytest.raises(capi.FastHevcError):
        ctx.motion_amvp(ins["nodes"][d], qp=52)
    assert ctx.stats()["kernels_launched"] == after["kernels_launched"]


@pytest.mark.parametrize("coarse", [0, mc.COARSE])
def test_p_tree_amvp_frame_equals_the_pieces(torch_cuda, coarse):
    """the two-motion pair through the one-call form, and through its pieces queued on one stream, zero-centred and centred"""
    torch = torch_cuda
    cur, ref = mc.pictures()
    w, h, qp = mc.W, mc.H, mc.QP
    R = mc.CENTRED_RANGE if coarse else mc.RANGE
    MRG = mc.CENTRED_MERGE_RANGE if coarse else R
    c = capi.Context(w, h, 8, max_frames=2)
    n = c.num_ctus
    per = (85, 124, 384)
    d_luma = to_dev(torch, np.stack([ref, cur]))
    cen = Guarded(torch, n * 16)
    found, fine, priced = ([Guarded(torch, n * k * 16) for k in per] for _ in range(3))
    merge, shapes, dmin, dmax = Guarded(torch, n * 85 * 16), Guarded(torch, n * 85 * 16), Guarded(torch, n * 256), Guarded(torch, n * 256)
    mpu = [Guarded(torch, n * k * 16) for k in per[1:]]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, p = st.cuda_stream, d_luma.data_ptr()
    launched = c.stats()["kernels_launched"]
    if coarse:
        c.motion_centres_device(p, 1, w, w * h, 2, cen.ptr, stream=s, qp=qp, coarse_range=coarse)
        c.motion_search_pu_centred_device(p, 1, w, w * h, 2, cen.ptr, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
        c.motion_refine_pu_centred_device(p, 1, w, w * h, 2, cen.ptr, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s, qp=qp,
                                          max_range=R)
    else:
        c.motion_search_pu_wide_device(p, 1, w, w * h, 2, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
        c.motion_refine_pu_wide_device(p, 1, w, w * h, 2, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s, qp=qp, max_range=R)
    c.motion_amvp_device(2, fine[0].ptr, fine[1].ptr, fine[2].ptr, priced[0].ptr, priced[1].ptr, priced[2].ptr, stream=s, qp=qp)
    c.motion_merge_device(p, 1, w, w * h, 2, priced[0].ptr, merge.ptr, stream=s, qp=qp, max_range=MRG)
    c.motion_merge_pu_device(p, 1, w, w * h, 2, priced[0].ptr, mpu[0].ptr, mpu[1].ptr, stream=s, qp=qp, max_range=MRG)
    c.pu_shape_select_merge_device(priced[0].ptr, priced[1].ptr, priced[2].ptr, mpu[0].ptr, mpu[1].ptr, 1, shapes.ptr, stream=s)
    c.p_tree_select_merge_device(shapes.ptr, merge.ptr, 1, dmin.ptr, dmax.ptr, None, stream=s)
    torch.cuda.synchronize()
    piece_launches = c.stats()["kernels_launched"] - launched
    pieces = dict(merge=merge.result(MDT, (n, 85)), shapes=shapes.result(SDT, (n, 85)), dmin=dmin.result(np.uint8, (n, 256)), dmax=dmax.result(np.uint8, (n, 256)))
    # the re-pricing piece against the restatement, on the pieces' own refined entries
    refined = [g.result(QDT, (n, k)) for g, k in zip(fine, per)]
    exp = ar.expected_all(w, h, *refined, qp)
    for f, g, k in zip(FAMILIES, priced, per):
        ar.same(g.result(QDT, (n, k)), exp[f][0], ("pieces", f, coarse))
    assert any((exp[f][0]["cost_best"] != r["cost_best"]).any() for f, r in zip(FAMILIES, refined))
    # the one-call form
    bc, org, stride = pel(cur)
    br, _, _ = pel(ref)
    before = c.stats()
    lo, hi, sh, me = c.p_tree_amvp_frame(bc, br, org, stride, qp=qp, search_range=R, coarse_range=coarse, with_shapes=True, with_merge=True)
    after = c.stats()
    assert lo.tobytes() == pieces["dmin"].tobytes() and hi.tobytes() == pieces["dmax"].tobytes()
    assert sh.tobytes() == pieces["shapes"].tobytes() and me.tobytes() == pieces["merge"].tobytes()
    assert after["bytes_h2d"] - before["bytes_h2d"] == w * h * 4 and after["bytes_d2h"] - before["bytes_d2h"] == n * (512 + 2 * 85 * 16)
    assert after["kernels_launched"] - before["kernels_launched"] == piece_launches
    # one launch more than fhevc_p_tree_merge_pu_frame, whose records are those on the zero-predictor costs
    before = c.stats()
    _, _, sh0, _ = c.p_tree_merge_pu_frame(bc, br, org, stride, qp=qp, search_range=R, coarse_range=coarse, with_shapes=True, with_merge=True)
    assert c.stats()["kernels_launched"] - before["kernels_launched"] == piece_launches - 1
    assert (sh0["cost_best"] != sh["cost_best"]).any()
    launched = c.stats()["kernels_launched"]
    for change in (dict(search_range=9, coarse_range=1), dict(coarse_range=15), dict(search_range=65), dict(qp=52)):
        with pytest.raises(capi.FastHevcError):
            c.p_tree_amvp_frame(bc, br, org, stride, **dict(dict(qp=qp, search_range=R, coarse_range=coarse), **change))
    assert c.stats()["kernels_launched"] == launched
    c.close()


# ---- 5. rejected calls and the timing slot ---------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing_and_slot_25(torch_cuda, ctxs):
    torch = torch_cuda
    ins, _, _ = ar.draw_batch()
    ctx, lib = ctxs[8], ctxs[8].lib
    held = {f: at_offset(torch, ins[f][:1], 0) for f in FAMILIES}
    out, mvp = Guarded(torch, N * 384 * 16), Guarded(torch, N * 384 * 8)
    torch.cuda.synchronize()
    good = dict(ctx=ctx.h, nf=2, rb=0, re=CH, qp=30, nodes=held["nodes"][1], pus=held["pu"][1], small=held["small"][1], o_nodes=out.ptr, o_pus=None, o_small=None,
                m_nodes=None, m_pus=None, m_small=mvp.ptr)
    bad = [(dict(ctx=None), None), (dict(nodes=None), "refined nodes"), (dict(o_nodes=None, m_small=None), "at least one output"),
           (dict(pus=None, o_pus=out.ptr), "family"), (dict(small=None), "family"), (dict(pus=None, m_pus=mvp.ptr), "family"), (dict(nf=1), "layout"), (dict(qp=-1), "qp"),
           (dict(qp=52), "qp"), (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"), (dict(o_nodes=out.ptr + 2), "aligned"),
           (dict(nodes=held["nodes"][1] + 1), "aligned"), (dict(m_small=mvp.ptr + 2), "aligned")]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_amvp_device(a["ctx"], a["nf"], a["rb"], a["re"], a["qp"], a["nodes"], a["pus"], a["small"], a["o_nodes"], a["o_pus"], a["o_small"], a["m_nodes"],
                                            a["m_pus"], a["m_small"], None)
    for change, text in bad:
        assert call(dict(good, **change)) == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert out.untouched() and mvp.untouched() and ctx.stats()["kernels_launched"] == launched
    # the timing slot: one launch per call under 25, nothing under its neighbours' slots; 24 and 26 are no slots
    ctx.enable_kernel_timing(True)
    for s in (19, 21, 23, 25):
        ctx.kernel_timing(s, reset=True)
    for calls in (1, 2):
        assert call(good) == capi.OK
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(25)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (19, 21, 23))
    ctx.enable_kernel_timing(False)
    assert not out.untouched() and not mvp.untouched()
    for s in (24, 26):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
