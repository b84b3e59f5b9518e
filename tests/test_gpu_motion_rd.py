"""Config 4 (P slices): the RD stage (k_motion_rd.hip) and the tree on RD costs on the MI355X, byte for byte against the Python restatement
tests/motion_rd_ref.py, which tests/test_motion_rd_ref.py pins to the reference's own transforms and quantiser without a GPU.  Nothing is compared with
the kernel's own output except where two launches must give the same bytes; the two zero bits and the vector are also compared with the existing skip
kernel's on the same merge records.

Pictures are the restatement's draw, 168 x 152 = 3 x 3 CTUs: two whole CTUs in either direction, ragged in both, so the last column and row hold nodes
that are not INSIDE.  The reference planes and the expected records are computed once per (bit depth, range) and shared."""
import ctypes as C

import numpy as np
import pytest

import motion_refine_ref as mr
import motion_rd_ref as rd
import motion_skip_ref as sk
import p_tree_ref as tr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

W, H, CW, CH, N = rd.DRAW_W, rd.DRAW_H, rd.DRAW_CW, rd.DRAW_CH, rd.DRAW_N
MDT, QDT, PDT, RDT, KDT, TDT = capi.MOTION_MERGE_DTYPE, capi.MOTION_QPEL_DTYPE, capi.MOTION_MVP_DTYPE, capi.MOTION_RD_DTYPE, capi.MOTION_SKIP_DTYPE, capi.TREE_DTYPE
_CACHE = {}


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


def pictures(bd):
    """three pictures at bd bits: frame 1 is predicted from frame 0, frame 2 from frame 1"""
    if ("pics", bd) not in _CACHE:
        ref, cur = rd.draw_pictures(bd)
        _CACHE[("pics", bd)] = [ref, cur, rd.draw_pictures(bd, seed=1)[1]]
    return _CACHE[("pics", bd)]


def planes_of(bd, f, max_range):
    """the sixteen fractional planes of frame f, wide enough for max_range; computed once"""
    pad = 16 if max_range <= 8 else 72
    if ("planes", bd, f, pad) not in _CACHE:
        _CACHE[("planes", bd, f, pad)] = mr.Planes(pictures(bd)[f], bd, pad)
    return _CACHE[("planes", bd, f, pad)]


def expected_batch(bd, nf, qp, recs, source, max_range, mvp=None, rows=None):
    """recs [nf - 1, band CTUs, 85] compact over the band -> the RD records of the same shape"""
    out = np.zeros(recs.shape, RDT)
    pics = pictures(bd)
    for f in range(1, nf):
        out[f - 1] = rd.expected(pics[f], pics[f - 1], W, H, bd, qp, recs[f - 1], source, max_range, mvp=None if mvp is None else mvp[f - 1], rows=rows,
                                 planes=planes_of(bd, f - 1, max_range))
    return out


def records(source, seed, max_range, nf=2, with_mvp=False):
    return rd.draw_records(source, seed, max_range, shape=(nf - 1, N, 85), with_mvp=with_mvp)


def pel_batch(bd, nf):
    planes = [pel(p) for p in pictures(bd)[:nf]]
    return np.stack([p[0] for p in planes]), planes[0][1], planes[0][2], planes[0][0].size


def run_rd(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, source, recs, qp, max_range, mvp=None, rows=None, stream=None, offsets=(0, 0, 0)):
    """recs [nf - 1, band CTUs, 85] -> the RD records of the same shape; the output lies between canaries; offsets: of d_in, d_mvp, d_out behind 16 bytes"""
    d_luma = to_dev(torch, flat)
    held, p_in = at_offset(torch, recs, offsets[0])
    mheld, p_mvp = at_offset(torch, mvp, offsets[1]) if mvp is not None else (None, None)
    out = Guarded(torch, recs.size * 16, offsets[2])
    torch.cuda.synchronize()
    ctx.motion_rd_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, source, p_in, out.ptr, d_mvp=p_mvp, rows=rows, stream=stream,
                         qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    return out.result(RDT, recs.shape)


def band(a, rows):
    return np.ascontiguousarray(a[:, rows[0] * CW:rows[1] * CW])


def check_invalid(got, recs, max_range, mvp=None):
    """exactly the nodes that are not INSIDE, are marked, lie out of reach or have a marker predictor record carry the invalid record"""
    reach = 4 * max_range + 3
    for c in range(N):
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            n = 64 >> lvl
            ins = (c % CW) * 64 + (bx + 1) * n <= W and (c // CW) * 64 + (by + 1) * n <= H
            for f in range(got.shape[0]):
                r, m = got[f, c, k], recs[f, c, k]
                valid = ins and m["cost_best"] != rd.MARK and abs(int(m["mvx"])) <= reach and abs(int(m["mvy"])) <= reach and (mvp is None or mvp[f, c, k]["idx"] != 255)
                assert (tuple(r) == rd.INVALID) == (not valid), (c, k, r, m)
                assert not valid or ((r["mvx"], r["mvy"]) == (m["mvx"], m["mvy"]) and r["cost_rd"] <= rd.SAT and (r["flags"] & 2) <= 2 * (r["flags"] & 1))


# ---- 1. the kernel against the restatement: bit depths, plane types, both window layouts, the three kinds of input ------------------------------------------

@pytest.mark.parametrize("dtype,bd,max_range,qps", [(np.int16, 8, 8, (4, 22, 37)), (np.int16, 10, 33, (10, 27, 51)), (np.int16, 12, 64, (14, 22, 51)),
                                                    (np.uint8, 8, 64, (27, 4, 10)), (np.int16, 12, 8, (4, 37, 27))])
def test_kernel_equals_the_restatement(torch_cuda, dtype, bd, max_range, qps):
    """max_range 8: the MR = 8 layout; 33 and 64: the MR = 64 layout with a part of its window and with the whole of it staged.  Merge records, explicit
    records priced against the zero predictor, explicit records with predictor records"""
    sb = np.dtype(dtype).itemsize
    flat, origin, stride, fstride = frames.guarded_plane(pictures(bd), bit_depth=bd, dtype=dtype, poison=None)
    ctx = capi.Context(W, H, bd, max_frames=3)
    split_seen = whole_seen = zero_seen = 0
    for (source, with_mvp), qp in zip(((rd.MERGE, False), (rd.EXPLICIT, False), (rd.EXPLICIT, True)), qps):
        recs, mvp = records(source, 40 + bd + max_range + source, max_range, nf=3, with_mvp=with_mvp)
        got = run_rd(torch_cuda, ctx, flat, origin, stride, fstride, 3, sb, source, recs, qp, max_range, mvp=mvp)
        rd.same(got, expected_batch(bd, 3, qp, recs, source, max_range, mvp=mvp), (dtype.__name__, bd, max_range, source, with_mvp, qp))
        check_invalid(got, recs, max_range, mvp)
        ok = got["cost_rd"] != rd.MARK
        split_seen += int((got["tu_split"][ok] != 0).sum())
        whole_seen += int((got["tu_split"][ok] == 0).sum())
        zero_seen += int(((got["flags"][ok] & 1) != 0).sum())
        reach = 4 * max_range + 3
        assert (ok & (np.abs(got["mvx"]) == reach)).any() and (ok & (np.abs(got["mvy"]) == reach)).any()         # vectors on the limit of the reach were tested
    assert split_seen > 50 and whole_seen > 50 and zero_seen > 0
    ctx.close()


# ---- 2. bands, poisoned planes, pointers off 16, large batches, streams ------------------------------------------------------------------------------------

def test_bands_are_slices_and_an_empty_band(torch_cuda):
    torch = torch_cuda
    qp, R, bd = 27, 8, 10
    full, _ = records(rd.MERGE, 8, R, nf=3)
    flat, org, stride, fs = pel_batch(bd, 3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    whole = run_rd(torch, ctx, flat, org, stride, fs, 3, 2, rd.MERGE, full, qp, R)
    rd.same(whole, expected_batch(bd, 3, qp, full, rd.MERGE, R), "whole")
    for rows in ((1, 2), (1, 3), (0, 1)):
        got = run_rd(torch, ctx, flat, org, stride, fs, 3, 2, rd.MERGE, band(full, rows), qp, R, rows=rows)      # guards checked inside
        assert got.tobytes() == band(whole, rows).tobytes(), rows       # a node reads no neighbour: a band is exactly a slice
    d_luma, d_in, out = to_dev(torch, flat), to_dev(torch, full), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_rd_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, rd.MERGE, d_in.data_ptr(), out.ptr, rows=(2, 2), qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype,bd,max_range", [(np.int16, 10, 8), (np.uint8, 8, 33), (np.int16, 12, 64)])
def test_guarded_planes_poisoned_margins_odd_origin_and_stride(torch_cuda, dtype, bd, max_range):
    """nothing outside the picture is read for its value: the margins, the stride padding and the gap between frames hold poison; the origin and the
    stride are odd, so no row is aligned; the records land between canaries"""
    flat, origin, stride, fstride = frames.guarded_plane(pictures(bd), bit_depth=bd, dtype=dtype, extra_stride=3, shift=1, frame_gap=5, poison=77)
    assert stride % 2 == 1 and origin % 2 == 1
    recs, mvp = records(rd.EXPLICIT, bd + max_range, max_range, nf=3, with_mvp=True)
    ctx = capi.Context(W, H, bd, max_frames=3)
    got = run_rd(torch_cuda, ctx, flat, origin, stride, fstride, 3, np.dtype(dtype).itemsize, rd.EXPLICIT, recs, 22, max_range, mvp=mvp)
    rd.same(got, expected_batch(bd, 3, 22, recs, rd.EXPLICIT, max_range, mvp=mvp), (dtype.__name__, bd, max_range))
    check_invalid(got, recs, max_range, mvp)
    ctx.close()


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_pointers_off_their_16_byte_alignment(torch_cuda, offset):
    """d_in, d_mvp and d_out 4, 8, 12 bytes behind a 16-byte boundary, one at a time and all together: the same bytes"""
    bd, R, qp = 8, 8, 14
    recs, mvp = records(rd.EXPLICIT, 77, R, with_mvp=True)
    flat, org, stride, fs = pel_batch(bd, 2)
    ctx = capi.Context(W, H, bd, max_frames=2)
    aligned = run_rd(torch_cuda, ctx, flat, org, stride, fs, 2, 2, rd.EXPLICIT, recs, qp, R, mvp=mvp)
    rd.same(aligned, expected_batch(bd, 2, qp, recs, rd.EXPLICIT, R, mvp=mvp), "aligned")
    for offsets in ((offset, 0, 0), (0, offset, 0), (0, 0, offset), (offset, 16 - offset, offset)):
        got = run_rd(torch_cuda, ctx, flat, org, stride, fs, 2, 2, rd.EXPLICIT, recs, qp, R, mvp=mvp, offsets=offsets)
        assert got.tobytes() == aligned.tobytes(), offsets
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_more_ctus_than_the_persistent_grid(torch_cuda, max_range):
    """116 picture pairs of 9 CTUs = 1 044 CTUs in one launch, more than four workgroups on each of 256 CUs: two pictures alternate and the records repeat,
    so pair f equals pair f - 2; the first two pairs equal the restatement"""
    a, b = pictures(8)[:2]
    NF = 117
    assert (NF - 1) * N > 4 * 256
    one, _ = records(rd.MERGE, max_range, max_range, nf=2)
    two, _ = records(rd.MERGE, max_range + 1, max_range, nf=2)
    recs = np.concatenate([one, two])
    ctx = capi.Context(W, H, 8, max_frames=NF)
    flat = np.stack([a, b] * (NF // 2) + [a]).astype(np.uint8)
    got = run_rd(torch_cuda, ctx, flat, 0, W, W * H, NF, 1, rd.MERGE, np.tile(recs, (NF // 2, 1, 1)), 22, max_range)
    exp = np.zeros((2, N, 85), RDT)
    exp[0] = rd.expected(b, a, W, H, 8, 22, recs[0], rd.MERGE, max_range, planes=planes_of(8, 0, max_range))
    exp[1] = rd.expected(a, b, W, H, 8, 22, recs[1], rd.MERGE, max_range, planes=planes_of(8, 1, max_range))
    rd.same(got[:2], exp, "first pairs")
    first = got[:2].tobytes()
    for f in range(2, NF - 1, 2):
        assert got[f:f + 2].tobytes() == first, f
    ctx.close()


def test_two_streams_with_different_qps_ranges_and_sources(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, org, stride, fs = pel_batch(bd, 3)
    calls = []
    for i, (qp, R, source, with_mvp) in enumerate(((10, 8, rd.MERGE, False), (51, 64, rd.EXPLICIT, True), (27, 8, rd.EXPLICIT, False), (22, 33, rd.MERGE, False))):
        recs, mvp = records(source, 100 + i, R, nf=3, with_mvp=with_mvp)
        calls.append((qp, R, source, recs, mvp, expected_batch(bd, 3, qp, recs, source, R, mvp=mvp)))
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_in = [to_dev(torch, c[3]) for c in calls]
    d_mvp = [to_dev(torch, c[4]) if c[4] is not None else None for c in calls]
    outs = [Guarded(torch, c[3].size * 16) for c in calls]
    torch.cuda.synchronize()
    for i, (qp, R, source, _, _, _) in enumerate(calls):
        ctx.motion_rd_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, source, d_in[i].data_ptr(), outs[i].ptr,
                             d_mvp=d_mvp[i].data_ptr() if d_mvp[i] is not None else None, stream=streams[i % 2].cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    for i, c in enumerate(calls):
        rd.same(outs[i].result(RDT, c[3].shape), c[5], i)
    ctx.close()


# ---- 3. against the existing kernels ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,max_range", [(8, 8), (10, 64), (12, 8)])
def test_flag_bits_and_vector_equal_the_skip_kernels(torch_cuda, bd, max_range):
    torch = torch_cuda
    flat, org, stride, fs = pel_batch(bd, 3)
    recs, _ = records(rd.MERGE, 300 + bd, max_range, nf=3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, d_in = to_dev(torch, flat), to_dev(torch, recs)
    for qp in (4, 22, 37, 51):
        a, b = Guarded(torch, recs.size * 16), Guarded(torch, recs.size * 16)
        torch.cuda.synchronize()
        ctx.motion_rd_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, rd.MERGE, d_in.data_ptr(), a.ptr, qp=qp, max_range=max_range)
        ctx.motion_skip_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, d_in.data_ptr(), b.ptr, qp=qp, max_range=max_range)
        torch.cuda.synchronize()
        r, s = a.result(RDT, recs.shape), b.result(KDT, recs.shape)
        assert np.array_equal(r["cost_rd"] == rd.MARK, s["coef_max"] == sk.MARK)
        assert np.array_equal(r["flags"] & 3, s["flags"]) and np.array_equal(r["mvx"], s["mvx"]) and np.array_equal(r["mvy"], s["mvy"]), qp
    ctx.close()


def test_the_chain_on_one_stream_and_the_rd_tree(torch_cuda):
    """search -> refinement -> re-pricing -> merge -> the RD stage on the merge records and on the re-priced records with their predictor records -> the RD
    tree, all on one stream without a host synchronisation; every stage's output is then compared with the restatement on the device's own inputs, and
    the RD tree with the skip tree on the same bytes"""
    torch = torch_cuda
    bd, R, qp = 8, 8, 27
    ys = frames.pan_clip(W, H, 2, seed=39, v_structure=-5, v_noise=3)
    pics = [y.astype(np.int64) for y in ys]
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=np.uint8, poison=None)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    p = d_luma.data_ptr() + origin
    found, fine, priced, merge, rd_m, rd_e, tree = (Guarded(torch, N * 85 * 16) for _ in range(7))
    mvp, dmin, dmax = Guarded(torch, N * 85 * 8), Guarded(torch, N * 256), Guarded(torch, N * 256)
    skip_tree, smin, smax = Guarded(torch, N * 85 * 16), Guarded(torch, N * 256), Guarded(torch, N * 256)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = st.cuda_stream
    ctx.motion_search_pu_wide_device(p, 1, stride, fstride, 2, found.ptr, None, None, stream=s, qp=qp, search_range=R)
    ctx.motion_refine_device(p, 1, stride, fstride, 2, found.ptr, fine.ptr, stream=s, qp=qp, max_range=R)
    ctx.motion_amvp_device(2, fine.ptr, d_out_nodes=priced.ptr, d_mvp_nodes=mvp.ptr, stream=s, qp=qp)
    ctx.motion_merge_device(p, 1, stride, fstride, 2, priced.ptr, merge.ptr, stream=s, qp=qp, max_range=R)
    ctx.motion_rd_device(p, 1, stride, fstride, 2, rd.MERGE, merge.ptr, rd_m.ptr, stream=s, qp=qp, max_range=R)
    ctx.motion_rd_device(p, 1, stride, fstride, 2, rd.EXPLICIT, priced.ptr, rd_e.ptr, d_mvp=mvp.ptr, stream=s, qp=qp, max_range=R)
    ctx.p_tree_select_rd_device(rd_e.ptr, rd_m.ptr, 3, 1, dmin.ptr, dmax.ptr, tree.ptr, stream=s)
    ctx.p_tree_select_skip_device(rd_e.ptr, rd_m.ptr, rd_m.ptr, 3, 1, smin.ptr, smax.ptr, skip_tree.ptr, stream=s)
    torch.cuda.synchronize()
    planes = mr.Planes(pics[0], bd, 16)
    m, q, v = merge.result(MDT, (1, N, 85)), priced.result(QDT, (1, N, 85)), mvp.result(PDT, (1, N, 85))
    got_m, got_e = rd_m.result(RDT, (1, N, 85)), rd_e.result(RDT, (1, N, 85))
    rd.same(got_m[0], rd.expected(pics[1], pics[0], W, H, bd, qp, m[0], rd.MERGE, R, planes=planes), "merge")
    rd.same(got_e[0], rd.expected(pics[1], pics[0], W, H, bd, qp, q[0], rd.EXPLICIT, R, mvp=v[0], planes=planes), "explicit")
    assert (got_e["cost_rd"] != rd.MARK).sum() > 300 and (got_m["cost_rd"] != rd.MARK).sum() > 300
    erec, emin, emax = rd.tree_select(got_e, got_m, 3, W, H)
    t = tree.result(TDT, (1, N, 85))
    tr.same(t, erec, "tree")
    assert np.array_equal(dmin.result(np.uint8, (1, N, 256)), emin) and np.array_equal(dmax.result(np.uint8, (1, N, 256)), emax)
    # ... and the skip tree's instance on the same bytes, reinterpreted
    assert skip_tree.result(TDT, (1, N, 85)).tobytes() == t.tobytes()
    assert smin.result(np.uint8, (N, 256)).tobytes() == dmin.result(np.uint8, (N, 256)).tobytes() and smax.result(np.uint8, (N, 256)).tobytes() == dmax.result(np.uint8, (N, 256)).tobytes()
    ctx.close()


def test_rd_tree_on_random_records_equals_the_skip_tree_and_the_restatement(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(29)
    a = np.frombuffer(rng.bytes(2 * N * 85 * 16), RDT).reshape(2, N, 85).copy()
    b = np.frombuffer(rng.bytes(2 * N * 85 * 16), RDT).reshape(2, N, 85).copy()
    for x in (a, b):
        x["cost_rd"] = np.where(rng.random(x.shape) < 1 / 7, rd.MARK, x["cost_rd"] % 100000)
    ctx = capi.Context(W, H, 8)
    for mask, rule, rows in ((0, None, None), (1, tr.random_rule(rng), None), (3, tr.random_rule(rng), (1, 3)), (2, capi.p_tree_rule_default(), (0, 1))):
        aa, bb = (a, b) if rows is None else (band(a, rows), band(b, rows))
        nb = aa.shape[1]
        (held_a, pa), (held_b, pb) = at_offset(torch, aa, 4), at_offset(torch, bb, 12)     # the tensors own the bytes until the results are down
        outs = [(Guarded(torch, 2 * nb * 256), Guarded(torch, 2 * nb * 256), Guarded(torch, 2 * nb * 85 * 16, 8)) for _ in range(2)]
        torch.cuda.synchronize()
        ctx.p_tree_select_rd_device(pa, pb, mask, 2, outs[0][0].ptr, outs[0][1].ptr, outs[0][2].ptr, rows=rows, rule=rule)
        ctx.p_tree_select_skip_device(pa, pb, pb, mask, 2, outs[1][0].ptr, outs[1][1].ptr, outs[1][2].ptr, rows=rows, rule=rule)
        torch.cuda.synchronize()
        erec, emin, emax = rd.tree_select(aa, bb, mask, W, H, rows=rows, rule=rule)
        got = outs[0][2].result(TDT, (2, nb, 85))
        tr.same(got, erec, (mask, rows))
        assert np.array_equal(outs[0][0].result(np.uint8, (2, nb, 256)), emin) and np.array_equal(outs[0][1].result(np.uint8, (2, nb, 256)), emax)
        assert got.tobytes() == outs[1][2].result(TDT, (2, nb, 85)).tobytes()
        if mask:
            assert ((erec["flags"] & sk.SKIPPED) != 0).any()
    ctx.close()


# ---- 4. the host form, rejected calls, the timing slot ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_range,source,with_mvp", [(8, rd.MERGE, False), (64, rd.EXPLICIT, True), (8, rd.EXPLICIT, False)])
def test_host_form_equals_device_form_and_counts_what_it_moves(torch_cuda, max_range, source, with_mvp):
    bd = 10
    recs, mvp = records(source, 3, max_range, with_mvp=with_mvp)
    planes = [pel(p) for p in pictures(bd)[:2]]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, bd, max_frames=2)
    dev = run_rd(torch_cuda, ctx, np.stack([p[0] for p in planes]), org, stride, fs, 2, 2, source, recs, 22, max_range, mvp=mvp)
    before = ctx.stats()
    host = ctx.motion_rd(planes[1][0], planes[0][0], recs[0], source, mvp=None if mvp is None else mvp[0], origin=org, stride=stride, qp=22, max_range=max_range)
    after = ctx.stats()
    assert host.tobytes() == dev[0].tobytes() and (host["cost_rd"] != rd.MARK).sum() > 200
    assert after["bytes_h2d"] - before["bytes_h2d"] == 4 * W * H + N * 85 * (24 if with_mvp else 16) and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    # a rejected call moves nothing
    with pytest.raises(capi.FastHevcError):
        ctx.motion_rd(planes[1][0], planes[0][0], recs[0], source, origin=org, stride=stride, qp=52, max_range=max_range)
    assert ctx.stats() == after
    ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, org, stride, fs = pel_batch(bd, 3)
    full, mvp = records(rd.EXPLICIT, 8, 8, nf=3, with_mvp=True)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, d_in, d_mvp, out = to_dev(torch, flat), to_dev(torch, full), to_dev(torch, mvp), Guarded(torch, full.size * 16)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr() + 2 * org, sb=2, stride=stride, fs=fs, nf=3, rb=0, re=CH, qp=30, R=8, source=1, rec=d_in.data_ptr(), mvp=d_mvp.data_ptr(),
                out=out.ptr)
    bad = [(dict(ctx=None), None), (dict(luma=None), "argument"), (dict(rec=None), "argument"), (dict(out=None), "argument"), (dict(nf=1), "layout"),
           (dict(sb=3), "layout"), (dict(stride=W - 1), "layout"), (dict(qp=-1), "qp"), (dict(qp=52), "qp"), (dict(R=0), "max_range"), (dict(R=65), "max_range"),
           (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"), (dict(sb=1), "uint8"), (dict(fs=stride), "overlap"),
           (dict(source=-1), "source"), (dict(source=2), "source"), (dict(source=0), "explicit source"), (dict(rec=d_in.data_ptr() + 2), "aligned"),
           (dict(mvp=d_mvp.data_ptr() + 1), "aligned"), (dict(out=out.ptr + 2), "aligned")]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_rd_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["source"], a["rec"], a["mvp"],
                                          a["out"], None)
    for change, text in bad:
        assert call(dict(good, **change)) == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    planes = [pel(p) for p in pictures(bd)[:2]]
    canary = np.full((N, 85), CANARY, np.uint8).repeat(16, axis=1).view(RDT)
    for change in (dict(qp=52), dict(max_range=0), dict(max_range=65), dict(source=2), dict(source=0)):
        res = canary.copy()
        kw = dict(dict(qp=30, max_range=8, source=1), **change)
        rc = lib.fhevc_motion_rd(ctx.h, planes[1][0].ctypes.data + 2 * org, planes[0][0].ctypes.data + 2 * org, stride, kw["qp"], kw["max_range"], kw["source"],
                                 full[0].ctypes.data, mvp[0].ctypes.data, res.ctypes.data)
        assert rc == capi.E_INVALID and res.tobytes() == canary.tobytes(), change
    assert ctx.stats()["kernels_launched"] == launched
    # what the skip tree rejects, the RD tree rejects
    for args in ((ctx.h, None, d_in.data_ptr(), 1, 2, 0, CH, None, out.ptr, None, None, None), (ctx.h, d_in.data_ptr(), None, 1, 2, 0, CH, None, out.ptr, None, None, None),
                 (ctx.h, d_in.data_ptr(), d_in.data_ptr(), 4, 2, 0, CH, None, out.ptr, None, None, None), (ctx.h, d_in.data_ptr(), d_in.data_ptr(), 1, 2, 0, CH, None, None, None, None, None),
                 (ctx.h, d_in.data_ptr(), d_in.data_ptr(), 1, 2, 0, CH + 1, None, out.ptr, None, None, None)):
        assert lib.fhevc_p_tree_select_rd_device(*args) == capi.E_INVALID, args
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    assert call(good) == capi.OK                  # the same call with nothing wrong is accepted
    torch.cuda.synchronize()
    assert not out.untouched()
    ctx.close()


def test_slot_29_counts_one_launch_per_call_and_28_stays_rejected(torch_cuda):
    torch = torch_cuda
    bd = 10
    flat, org, stride, fs = pel_batch(bd, 3)
    full, _ = records(rd.MERGE, 8, 8, nf=3)
    ctx = capi.Context(W, H, bd, max_frames=3)
    d_luma, d_in, out = to_dev(torch, flat), to_dev(torch, full), Guarded(torch, full.size * 16)
    dmin = Guarded(torch, 2 * N * 256)
    torch.cuda.synchronize()
    ctx.enable_kernel_timing(True)
    for s in (17, 19, 23, 27, 29):
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls, R in ((1, 8), (2, 64), (3, 8)):
        ctx.motion_rd_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, rd.MERGE, d_in.data_ptr(), out.ptr, qp=30, max_range=R)
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(29)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (17, 19, 23, 27))
    ctx.p_tree_select_rd_device(out.ptr, out.ptr, 3, 2, dmin.ptr)          # the RD tree is timed as the tree
    torch.cuda.synchronize()
    assert ctx.kernel_timing(17)[1] == 1 and ctx.kernel_timing(29)[1] == 3
    ctx.enable_kernel_timing(False)
    for s in (28, 30):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()
