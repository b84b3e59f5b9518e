"""Config 4 (P slices): the merge stage per PU (k_motion_merge_pu.hip), the partition-size selection that takes its costs (the merge instantiation of
k_pu_shape.hip) and fhevc_p_tree_merge_pu_frame on the MI355X, bit for bit and field by field against the Python restatement
tests/motion_merge_pu_ref.py (pinned without a GPU by tests/test_motion_merge_pu_ref.py).  Nothing is compared with a kernel's own output except where two
launches must give the same bytes.

Pictures are 200 x 136 = 4 x 3 CTUs, ragged by 8 samples on both sides, so candidates cross CTU borders into all four neighbour CTUs and the last column
and row hold CUs that are not INSIDE; the constructed cases bring their own sizes (tests/motion_merge_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import motion_merge_cases as mc
import motion_merge_pu_ref as mpr
import motion_merge_ref as mg
import motion_refine_ref as mr
import pu_shape_ref as sr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, clip_planes, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

W, H = 200, 136
CW, CH = 4, 3
N = CW * CH
MDT, QDT, SDT = capi.MOTION_MERGE_DTYPE, capi.MOTION_QPEL_DTYPE, capi.SHAPE_DTYPE
PER = {"pu": 124, "small": 384}
BOTH = ("pu", "small")
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


def band(a, rows):
    return np.ascontiguousarray(a[:, rows[0] * CW:rows[1] * CW])


def run_stage(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, refined, qp, max_range, rows=None, stream=None, families=BOTH):
    """refined [nf - 1, band CTUs, 85] -> {family: [nf - 1, band CTUs, 124 or 384]} for the families asked for; the outputs lie between canaries, and a
    family that was not asked for gets no pointer"""
    d_luma, d_ref = to_dev(torch, flat), to_dev(torch, refined)
    P, nb = refined.shape[:2]
    outs = {f: Guarded(torch, P * nb * PER[f] * 16) for f in families}
    torch.cuda.synchronize()
    ctx.motion_merge_pu_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, d_ref.data_ptr(), outs["pu"].ptr if "pu" in outs else None,
                               outs["small"].ptr if "small" in outs else None, rows=rows, stream=stream, qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    return {f: g.result(MDT, (P, nb, PER[f])) for f, g in outs.items()}


def expected_batch(oracle, pics, bd, qp, refined, max_range, rows=None, w=W, h=H, families=BOTH):
    """pics: [H, W] samples per frame; refined [nf - 1, band CTUs, 85] compact over the band -> {family: records}"""
    out = {f: np.zeros(refined.shape[:2] + (PER[f],), MDT) for f in families}
    for fr in range(1, len(pics)):
        buf, org, stride = pel(pics[fr])
        planes = mr.Planes(pics[fr - 1], bd, max_range + 8)
        for f in families:
            out[f][fr - 1] = mpr.expected(oracle, buf.reshape(-1), org, stride, pics[fr - 1], w, h, bd, qp, refined[fr - 1], max_range, f, rows=rows, planes=planes)
    return out


def same_all(got, exp, what):
    assert set(got) == set(exp)
    for f in got:
        mpr.same(got[f], exp[f], (what, f))


def check_markers(got):
    """PUs whose CU is not INSIDE carry the marker record, all others a list"""
    for f, a in got.items():
        cov = mpr.FAMILIES[f][0]()
        for c in range(N):
            for e, (k, s, p) in enumerate(cov):
                lvl, (gx, gy), _ = mpr.pu_geometry(W, c, k, s, p)
                ins = mg.inside(W, H, lvl, gx, gy)
                for r in a[:, c, e]:
                    assert (tuple(r) == mg.INVALID) == (not ins) and (1 <= r["num"] <= 5) == ins and r["pad"] == 0, (f, c, k, s, p, r)


def noise_pictures(seed, nf, bd=8):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, size=(H, W)).astype(np.int64) for _ in range(nf)]


# ---- 1. the real chain: search -> refinement -> stage on one stream, no host synchronisation ---------------------------------------------------------------

@pytest.mark.parametrize("dtype,bd", [(np.int16, 8), (np.int16, 10), (np.int16, 12), (np.uint8, 8)])
def test_real_chain_on_one_stream(oracle, torch_cuda, dtype, bd):
    """max_range 8: the MR = 8 layout; 33 and 64: the MR = 64 layout with a part of its window and with the whole of it staged; the three arithmetic forms"""
    torch = torch_cuda
    qp = {8: 27, 10: 32, 12: 22}[bd]
    ys = frames.pan_clip(W, H, 2, seed=31 + bd, v_structure=-5, v_noise=3)
    pics = clip_planes(ys, bd, low_bits_seed=5)
    sb = np.dtype(dtype).itemsize
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, poison=None)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    p = d_luma.data_ptr() + sb * origin
    for R in (8, 33, 64):
        found, fine = Guarded(torch, N * 85 * 16), Guarded(torch, N * 85 * 16)
        outs = {f: Guarded(torch, N * PER[f] * 16) for f in BOTH}
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = st.cuda_stream
        ctx.motion_search_pu_wide_device(p, sb, stride, fstride, 2, found.ptr, None, None, stream=s, qp=qp, search_range=R)
        ctx.motion_refine_device(p, sb, stride, fstride, 2, found.ptr, fine.ptr, stream=s, qp=qp, max_range=R)
        ctx.motion_merge_pu_device(p, sb, stride, fstride, 2, fine.ptr, outs["pu"].ptr, outs["small"].ptr, stream=s, qp=qp, max_range=R)
        torch.cuda.synchronize()
        refined = fine.result(QDT, (1, N, 85))
        got = {f: outs[f].result(MDT, (1, N, PER[f])) for f in BOTH}
        same_all(got, expected_batch(oracle, pics, bd, qp, refined, R), (dtype.__name__, bd, R))
        check_markers(got)
        for f in BOTH:
            ok = got[f]["num"] > 0
            assert (got[f]["src"][ok] != mg.ZERO).sum() > 200 and (got[f]["num"][ok] >= 2).any()
    ctx.close()


# ---- 2. the random-record draw of the CPU test, and the NULL combinations ------------------------------------------------------------------------------------

def draw_case(oracle):
    if "draw" not in _CACHE:
        pics, refined = mpr.random_draw()
        exp = expected_batch(oracle, pics, 8, mpr.DRAW_QP, refined[None], mpr.DRAW_RANGE)
        _CACHE["draw"] = (pics, refined[None], exp)
    return _CACHE["draw"]


def test_random_refined_records(oracle, torch_cuda):
    pics, refined, exp = draw_case(oracle)
    assert (mpr.DRAW_W, mpr.DRAW_H) == (W, H)
    ctx = capi.Context(W, H, 8, max_frames=2)
    got = run_stage(torch_cuda, ctx, np.stack(pics).astype(np.uint8), 0, W, W * H, 2, 1, refined, mpr.DRAW_QP, mpr.DRAW_RANGE)
    same_all(got, exp, "draw")
    check_markers(got)
    for f in BOTH:
        mpr.check_draw(refined[0], got[f][0], f)
    ctx.close()


def test_each_family_alone(oracle, torch_cuda):
    """d_out_pus or d_out_pus_small NULL: the other family's bytes are what they are when both are asked for"""
    pics, refined, exp = draw_case(oracle)
    ctx = capi.Context(W, H, 8, max_frames=2)
    for f in BOTH:
        got = run_stage(torch_cuda, ctx, np.stack(pics).astype(np.uint8), 0, W, W * H, 2, 1, refined, mpr.DRAW_QP, mpr.DRAW_RANGE, families=(f,))
        same_all(got, {f: exp[f]}, f)
    ctx.close()


# ---- 3. constructed pictures: expected values known in advance -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,fx,fy,mv", mc.HALF_CASES)
def test_a_half_sample_picture_merges_at_no_distortion(oracle, torch_cuda, bd, fx, fy, mv):
    case = mc.half_sample_case(bd, fx, fy, mv)
    (rb, org, stride), (cb, _, _) = pel(case["ref"]), pel(case["cur"])
    ctx = capi.Context(mc.HALF_W, mc.HALF_H, bd)
    got = dict(zip(BOTH, ctx.motion_merge_pu(cb, rb, case["refined"], org, stride, qp=mc.HALF_QP, max_range=8)))
    c1 = mg.bit_cost(1, mr.sqrt_lambda(oracle, mc.HALF_QP, bd))
    for f in BOTH:
        mpr.check_half_sample(got[f], f, mc.HALF_W, mc.HALF_H, case["q"], c1)
        mpr.same(got[f], mpr.expected(oracle, cb.reshape(-1), org, stride, case["ref"], mc.HALF_W, mc.HALF_H, bd, mc.HALF_QP, case["refined"], 8, f, planes=case["planes"]), f)
    ctx.close()


def test_two_motions_split_at_a_ctu_boundary(oracle, torch_cuda):
    """the two-motion pair as uint8 planes: the wide search at range 4, both refinements and the stage queued on one stream"""
    torch = torch_cuda
    cur, ref = mc.pictures()
    w, h, qp, R = mc.W, mc.H, mc.QP, mc.RANGE
    case = mc.two_motion_case(oracle)
    d_luma = to_dev(torch, np.stack([ref, cur]))
    c = capi.Context(w, h, 8, max_frames=2)
    n = c.num_ctus
    found = [Guarded(torch, n * k * 16) for k in (85, 124, 384)]
    fine = [Guarded(torch, n * k * 16) for k in (85, 124, 384)]
    outs = {f: Guarded(torch, n * PER[f] * 16) for f in BOTH}
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, p = st.cuda_stream, d_luma.data_ptr()
    c.motion_search_pu_wide_device(p, 1, w, w * h, 2, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
    c.motion_refine_pu_wide_device(p, 1, w, w * h, 2, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s, qp=qp, max_range=R)
    c.motion_merge_pu_device(p, 1, w, w * h, 2, fine[0].ptr, outs["pu"].ptr, outs["small"].ptr, stream=s, qp=qp, max_range=R)
    torch.cuda.synchronize()
    refined = fine[0].result(QDT, (n, 85))
    for f in QDT.names:
        assert np.array_equal(refined[f], case["refined"]["nodes"][f]), f
    got = {f: outs[f].result(MDT, (n, PER[f])) for f in BOTH}
    flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
    for f in BOTH:
        mpr.same(got[f], mpr.expected(oracle, flat, 0, w, ref.astype(np.int64), w, h, 8, qp, case["refined"]["nodes"], R, f), f)
    mpr.check_two_motions(got["pu"], fine[1].result(QDT, (n, 124)), (4 * mc.V2[0], 4 * mc.V2[1]), case["c"])
    c.close()


# ---- 4. bands, guarded planes, large batches, streams, the host form --------------------------------------------------------------------------------------------

def banded_case():
    if "banded" not in _CACHE:
        ys = frames.pan_clip(W, H, 3, seed=12, v_structure=4, v_noise=-3)
        pics = clip_planes(ys, 10, low_bits_seed=4)
        refined = mpr.random_refined(np.random.default_rng(8), (2, N, 85), 8)
        _CACHE["banded"] = (pics, refined)
    return _CACHE["banded"]


def admitted_from_above(full, rows, R, family):
    """[band CTUs, entries] bool: the whole picture's list of the PU holds a candidate from a CTU row above the band"""
    cov = mpr.FAMILIES[family][0]()
    nb = (rows[1] - rows[0]) * CW
    out = np.zeros((nb, len(cov)), bool)
    for i in range(nb):
        c = rows[0] * CW + i
        for e, (k, s, p) in enumerate(cov):
            lvl, (gx, gy), _ = mpr.pu_geometry(W, c, k, s, p)
            if not mg.inside(W, H, lvl, gx, gy):
                continue
            nbs = mpr.candidates(W, H, (0, CH), c, k, s, p)
            cands = [None if x is None else tuple(int(full[x[0], x[1]][f]) for f in ("cost_best", "mvx", "mvy")) for x in nbs]
            out[i, e] = any(src != mg.ZERO and nbs[src][0] < rows[0] * CW for src, _ in mg.build_list(cands, R))
    return out


def test_bands_between_canaries_and_an_empty_band(oracle, torch_cuda):
    torch = torch_cuda
    qp, R = 33, 8
    pics, full = banded_case()
    pics, full = pics[:2], full[:1]
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    ctx = capi.Context(W, H, 10, max_frames=2)
    whole = run_stage(torch, ctx, flat, org, stride, fs, 2, 2, full, qp, R)
    same_all(whole, expected_batch(oracle, pics, 10, qp, full, R), "whole")
    for rows in ((1, 2), (1, 3)):
        part = band(full, rows)
        got = run_stage(torch, ctx, flat, org, stride, fs, 2, 2, part, qp, R, rows=rows)      # guards checked inside
        same_all(got, expected_batch(oracle, pics, 10, qp, part, R, rows=rows), rows)
        # a band is a slice: its records differ from the whole picture's exactly where a candidate from the CTU row above was admitted to the whole picture's list
        for f in BOTH:
            differs = np.zeros(got[f].shape, bool)
            for name in MDT.names:
                differs |= got[f][name] != band(whole[f], rows)[name]
            above = admitted_from_above(full[0], rows, R, f)
            assert above.any() and np.array_equal(differs[0], above), (rows, f, int(differs.sum()), int(above.sum()))
            assert not above[CW:].any()           # only the band's first CTU row
    # an empty band writes nothing, launches nothing and succeeds
    d_luma, d_ref, out = to_dev(torch, flat), to_dev(torch, full), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_merge_pu_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 2, d_ref.data_ptr(), out.ptr, out.ptr, rows=(2, 2), qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype,bd,max_range", [(np.int16, 10, 8), (np.uint8, 8, 33), (np.int16, 12, 64)])
def test_guarded_planes_poisoned_margins_odd_origin_and_stride(oracle, torch_cuda, dtype, bd, max_range):
    """nothing outside the picture is read for its value: the margins, the stride padding and the gap between frames hold poison; the origin and the
    stride are odd, so no row is aligned; the records land between canaries"""
    qp = 27
    ys = frames.pan_clip(W, H, 2, seed=9, v_structure=-4, v_noise=6)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3, shift=1, frame_gap=5, poison=77)
    assert stride % 2 == 1 and origin % 2 == 1
    refined = mpr.random_refined(np.random.default_rng(bd + max_range), (1, N, 85), max_range)
    ctx = capi.Context(W, H, bd, max_frames=2)
    got = run_stage(torch_cuda, ctx, flat, origin, stride, fstride, 2, np.dtype(dtype).itemsize, refined, qp, max_range)
    same_all(got, expected_batch(oracle, pics, bd, qp, refined, max_range), (dtype.__name__, bd, max_range))
    check_markers(got)
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_more_ctus_than_the_persistent_grid(oracle, torch_cuda, max_range):
    """90 picture pairs of 12 CTUs = 1 080 CTUs in one launch, more than four workgroups on each of 256 CUs (the kernel's registers allow two): two pictures
    alternate and the refined records repeat, so pair f equals pair f - 2; the first two pairs equal the restatement"""
    a, b = noise_pictures(90 + max_range, 2)
    NF = 91
    assert (NF - 1) * N > 4 * 256
    refined = mpr.random_refined(np.random.default_rng(max_range), (2, N, 85), max_range)
    ctx = capi.Context(W, H, 8, max_frames=NF)
    flat = np.stack([a, b] * (NF // 2) + [a]).astype(np.uint8)
    got = run_stage(torch_cuda, ctx, flat, 0, W, W * H, NF, 1, np.tile(refined, (NF // 2, 1, 1)), 30, max_range)
    same_all({f: g[:2] for f, g in got.items()}, expected_batch(oracle, [a, b, a], 8, 30, refined, max_range), "first pairs")
    for f in BOTH:
        first = got[f][:2].tobytes()
        for fr in range(2, NF - 1, 2):
            assert got[f][fr:fr + 2].tobytes() == first, (f, fr)
    ctx.close()


def test_two_streams_with_different_qps_and_ranges(oracle, torch_cuda):
    torch = torch_cuda
    pics, _ = banded_case()
    pics = pics[:2]
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    calls = []
    for i, (qp, R) in enumerate(((12, 8), (47, 64), (30, 8), (22, 33))):
        refined = mpr.random_refined(np.random.default_rng(100 + i), (1, N, 85), R)
        calls.append((qp, R, refined, expected_batch(oracle, pics, 10, qp, refined, R)))
    ctx = capi.Context(W, H, 10, max_frames=2)
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_ref = [to_dev(torch, c[2]) for c in calls]
    outs = [{f: Guarded(torch, N * PER[f] * 16) for f in BOTH} for _ in calls]
    torch.cuda.synchronize()
    for i, (qp, R, _, _) in enumerate(calls):
        ctx.motion_merge_pu_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 2, d_ref[i].data_ptr(), outs[i]["pu"].ptr, outs[i]["small"].ptr,
                                   stream=streams[i % 2].cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    for i, c in enumerate(calls):
        same_all({f: outs[i][f].result(MDT, (1, N, PER[f])) for f in BOTH}, c[3], i)
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_host_form_equals_device_form(torch_cuda, max_range):
    pics, _ = banded_case()
    refined = mpr.random_refined(np.random.default_rng(3), (1, N, 85), max_range)
    planes = [pel(p) for p in pics[:2]]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=2)
    dev = run_stage(torch_cuda, ctx, np.stack([p[0] for p in planes]), org, stride, fs, 2, 2, refined, 25, max_range)
    before = ctx.stats()
    host = dict(zip(BOTH, ctx.motion_merge_pu(planes[1][0], planes[0][0], refined[0], org, stride, qp=25, max_range=max_range)))
    after = ctx.stats()
    for f in BOTH:
        assert host[f].tobytes() == dev[f][0].tobytes() and (host[f]["num"] > 0).sum() > 500
    # the pair and the refined nodes up, both families down, one launch
    assert after["bytes_h2d"] - before["bytes_h2d"] == W * H * 4 + N * 85 * 16 and after["bytes_d2h"] - before["bytes_d2h"] == N * 508 * 16
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    # one family alone: the same bytes, only that family comes back
    before = after
    only, none = ctx.motion_merge_pu(planes[1][0], planes[0][0], refined[0], org, stride, qp=25, max_range=max_range, with_small=False)
    assert none is None and only.tobytes() == host["pu"].tobytes() and ctx.stats()["bytes_d2h"] - before["bytes_d2h"] == N * 124 * 16
    none, only = ctx.motion_merge_pu(planes[1][0], planes[0][0], refined[0], org, stride, qp=25, max_range=max_range, with_pus=False)
    assert none is None and only.tobytes() == host["small"].tobytes()
    ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    pics, full = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=3)
    d_luma, d_ref = to_dev(torch, np.stack([p[0] for p in planes])), to_dev(torch, full)
    out, out_s = Guarded(torch, 2 * N * 124 * 16), Guarded(torch, 2 * N * 384 * 16)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr() + 2 * org, sb=2, stride=stride, fs=fs, nf=3, rb=0, re=CH, qp=30, R=8, ref=d_ref.data_ptr(), out=out.ptr, out_s=out_s.ptr)
    bad = [(dict(ctx=None), None), (dict(luma=None), "argument"), (dict(ref=None), "argument"), (dict(out=None, out_s=None), "argument"), (dict(nf=1), "layout"),
           (dict(sb=3), "layout"), (dict(stride=W - 1), "layout"), (dict(qp=-1), "qp"), (dict(qp=52), "qp"), (dict(R=0), "max_range"), (dict(R=65), "max_range"),
           (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"), (dict(sb=1), "uint8"), (dict(fs=stride), "overlap")]
    call = lambda a: lib.fhevc_motion_merge_pu_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["ref"], a["out"],
                                                      a["out_s"], None)
    launched = ctx.stats()["kernels_launched"]
    for change, text in bad:
        assert call(dict(good, **change)) == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
        # fhevc_motion_merge_device rejects the same call
        a = dict(good, **change)
        assert lib.fhevc_motion_merge_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["ref"],
                                             a["out"] if (a["out"] or a["out_s"]) else None, None) == capi.E_INVALID, change
    torch.cuda.synchronize()
    assert out.untouched() and out_s.untouched() and ctx.stats()["kernels_launched"] == launched
    # the host form
    canary = np.full((N, 124), CANARY, np.uint8).repeat(16, axis=1).view(MDT)
    for change in (dict(qp=52), dict(max_range=0), dict(max_range=65)):
        res = canary.copy()
        kw = dict(dict(qp=30, max_range=8), **change)
        rc = lib.fhevc_motion_merge_pu(ctx.h, planes[1][0].ctypes.data + 2 * org, planes[0][0].ctypes.data + 2 * org, stride, kw["qp"], kw["max_range"], full[0].ctypes.data,
                                       res.ctypes.data, None)
        assert rc == capi.E_INVALID and res.tobytes() == canary.tobytes(), change
    assert lib.fhevc_motion_merge_pu(ctx.h, planes[1][0].ctypes.data + 2 * org, planes[0][0].ctypes.data + 2 * org, stride, 30, 8, full[0].ctypes.data, None, None) == capi.E_INVALID
    assert ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted
    assert call(good) == capi.OK
    torch.cuda.synchronize()
    assert not out.untouched() and not out_s.untouched()
    ctx.close()


def test_slot_21_counts_one_launch_per_call(torch_cuda):
    torch = torch_cuda
    pics, full = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=3)
    d_luma, d_ref = to_dev(torch, np.stack([p[0] for p in planes])), to_dev(torch, full)
    out, out_s = Guarded(torch, 2 * N * 124 * 16), Guarded(torch, 2 * N * 384 * 16)
    torch.cuda.synchronize()
    ctx.enable_kernel_timing(True)
    for s in (7, 12, 13, 15, 17, 19, 21):
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls, R, ptrs in ((1, 8, (out.ptr, out_s.ptr)), (2, 64, (out.ptr, None)), (3, 8, (None, out_s.ptr))):
        ctx.motion_merge_pu_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, d_ref.data_ptr(), *ptrs, qp=30, max_range=R)
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(21)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (7, 12, 13, 15, 17, 19))
    ctx.enable_kernel_timing(False)
    for s in (20, 22):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()


# ---- 5. the selection with merge costs ------------------------------------------------------------------------------------------------------------------------------

def select_case():
    """random entries and merge records of the 200 x 136 context, two pictures, four rules, and their expected records, costs and bits; computed once"""
    if "select" not in _CACHE:
        rng = np.random.default_rng(911)
        nodes, pus, small = sr.random_entries(rng, 2, N)
        mpus, msmall = mpr.random_pu_merge(rng, pus, small)
        rules = {"default": None, "r1": sr.random_rule(rng, 0), "r2": sr.random_rule(rng, 1), "r3": sr.random_rule(rng, 1)}
        exp = {k: mpr.select(nodes, pus, small, mpus, msmall, W, H, rule=r) for k, r in rules.items()}
        _CACHE["select"] = ((nodes, pus, small, mpus, msmall), rules, exp)
    return _CACHE["select"]


def run_select(torch, ctx, arrays, rule, rows=None, want_costs=True, want_merged=True, offsets=(0,) * 5, shapes_offset=0, costs_offset=0, merged_offset=0, plain=False):
    """one call, then a synchronise -> (records, costs, merged), None for an output not asked for; guards checked.  arrays: nodes, pus, small, merge pus, merge
    small -- small and merge small may be None.  plain: fhevc_pu_shape_select_device on the refined entries alone"""
    P, nb = arrays[0].shape[:2]
    held = [None if a is None else at_offset(torch, a, o) for a, o in zip(arrays, offsets)]
    ptr = [None if x is None else x[1] for x in held]
    shapes, costs, merged = Guarded(torch, P * nb * 85 * 16, shapes_offset), Guarded(torch, P * nb * 85 * 32, costs_offset), Guarded(torch, P * nb * 85 * 2, merged_offset)
    torch.cuda.synchronize()
    if plain:
        ctx.pu_shape_select_device(ptr[0], ptr[1], ptr[2], P, shapes.ptr, costs.ptr if want_costs else None, rows=rows, rule=rule)
    else:
        ctx.pu_shape_select_merge_device(*ptr, P, shapes.ptr, costs.ptr if want_costs else None, merged.ptr if want_merged and not plain else None, rows=rows, rule=rule)
    torch.cuda.synchronize()
    assert want_costs or costs.untouched()
    assert (want_merged and not plain) or merged.untouched()
    return (shapes.result(SDT, (P, nb, 85)), costs.result(np.uint32, (P, nb, 85, 8)) if want_costs else None,
            merged.result(np.uint16, (P, nb, 85)) if want_merged and not plain else None)


def same_select(got, exp, what):
    sr.same(got[0], exp[0], what)
    if got[1] is not None:
        assert np.array_equal(got[1], exp[1]), (what, "costs", np.argwhere(got[1] != exp[1])[:5])
    if got[2] is not None:
        assert np.array_equal(got[2], exp[2]), (what, "merged", np.argwhere(got[2] != exp[2])[:5])


@pytest.fixture(scope="module")
def select_ctx(torch_cuda):
    c = capi.Context(W, H, 8)
    yield c
    c.close()


def test_selection_with_random_entries_and_merges(torch_cuda, select_ctx):
    arrays, rules, exp = select_case()
    seen = mpr.part_combinations(arrays[1], arrays[2], arrays[3], arrays[4], W, H)
    assert all(seen[l] == {(True, True), (True, False), (False, True), (False, False)} for l in range(4)), seen
    for rname, rule in rules.items():
        same_select(run_select(torch_cuda, select_ctx, arrays, rule), exp[rname], rname)
        for p in range(2):
            host = capi.pu_shape_select_merge(*(a[p] for a in arrays), W, H, rule, with_costs=True)
            same_select(host, tuple(e[p] for e in exp[rname]), ("host", rname, p))
    assert exp["r1"][2].any() and (exp["r1"][0]["best"] != sr.select(*arrays[:3], W, H, rule=rules["r1"])[0]["best"]).any()
    # NULL costs / merged / merge_pus_small / pus_small
    for wc, wm in ((True, False), (False, True), (False, False)):
        same_select(run_select(torch_cuda, select_ctx, arrays, rules["r2"], want_costs=wc, want_merged=wm), exp["r2"], (wc, wm))
    for keep_small, keep_msmall in ((True, False), (False, True), (False, False)):
        a = (arrays[0], arrays[1], arrays[2] if keep_small else None, arrays[3], arrays[4] if keep_msmall else None)
        same_select(run_select(torch_cuda, select_ctx, a, rules["r3"]), mpr.select(*a, W, H, rule=rules["r3"]), (keep_small, keep_msmall))
    # bands
    for rows in ((1, 2), (1, 3)):
        got = run_select(torch_cuda, select_ctx, tuple(band(a, rows) for a in arrays), rules["r3"], rows=rows)
        same_select(got, tuple(band(e, rows) for e in exp["r3"]), rows)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_selection_pointers_off_their_alignment(torch_cuda, select_ctx, offset):
    """the five inputs, d_shapes and d_costs 4, 8, 12 bytes behind a 16-byte boundary, d_merged 2, 4, 6 bytes: the same bytes"""
    arrays, rules, exp = select_case()
    aligned = run_select(torch_cuda, select_ctx, arrays, rules["r1"])
    same_select(aligned, exp["r1"], "aligned")
    o = 4 * offset
    for kw in (dict(offsets=(o, 0, 0, 0, 0)), dict(offsets=(0, o, 16 - o, 0, 0)), dict(offsets=(0, 0, 0, o, 16 - o)), dict(shapes_offset=o), dict(costs_offset=o),
               dict(merged_offset=2 * offset), dict(offsets=(o, 16 - o, o, 16 - o, o), shapes_offset=16 - o, costs_offset=o, merged_offset=2 * offset)):
        got = run_select(torch_cuda, select_ctx, arrays, rules["r1"], **kw)
        assert all(g.tobytes() == a.tobytes() for g, a in zip(got, aligned)), kw


def test_selection_with_all_merges_marked_is_the_plain_selection(torch_cuda, select_ctx):
    arrays, rules, _ = select_case()
    none_p, none_s = arrays[3].copy(), arrays[4].copy()
    none_p["cost_best"], none_s["cost_best"] = mg.MARK, mg.MARK          # every other byte stays random
    for rname in ("default", "r2"):
        b = run_select(torch_cuda, select_ctx, arrays, rules[rname], plain=True)
        for ms in (none_s, None):
            a = run_select(torch_cuda, select_ctx, arrays[:3] + (none_p, ms), rules[rname])
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and not a[2].any(), rname
    # slot 13 times both forms, slot 21 neither; a rejected call launches nothing
    select_ctx.enable_kernel_timing(True)
    select_ctx.kernel_timing(13, reset=True)
    select_ctx.kernel_timing(21, reset=True)
    run_select(torch_cuda, select_ctx, arrays, None)
    run_select(torch_cuda, select_ctx, arrays, None, plain=True)
    assert select_ctx.kernel_timing(13)[1] == 2 and select_ctx.kernel_timing(21)[1] == 0
    select_ctx.enable_kernel_timing(False)
    held, out = to_dev(torch_cuda, arrays[2]), Guarded(torch_cuda, 2 * N * 85 * 16)
    h, o = held.data_ptr(), out.ptr
    launched = select_ctx.stats()["kernels_launched"]
    lib = select_ctx.lib
    for args in ((select_ctx.h, h, h, h, None, h, 2, 0, CH, None, o, None, None, None), (select_ctx.h, None, h, h, h, h, 2, 0, CH, None, o, None, None, None),
                 (select_ctx.h, h, None, h, h, h, 2, 0, CH, None, o, None, None, None), (select_ctx.h, h, h, h, h, h, 2, 0, CH, None, None, None, None, None),
                 (select_ctx.h, h, h, h, h, h, 0, 0, CH, None, o, None, None, None), (select_ctx.h, h, h, h, h, h, 2, 0, CH + 1, None, o, None, None, None),
                 (select_ctx.h, h, h, h, h, h, 2, 0, CH, C.byref(capi.pu_shape_rule([0] * 4, [0] * 4, 2)), o, None, None, None)):
        assert lib.fhevc_pu_shape_select_merge_device(*args) == capi.E_INVALID, args
    torch_cuda.cuda.synchronize()
    assert out.untouched() and select_ctx.stats()["kernels_launched"] == launched
    # an empty band: accepted, nothing launched, nothing written
    assert lib.fhevc_pu_shape_select_merge_device(select_ctx.h, h, h, h, h, h, 2, 1, 1, None, o, None, None, None) == capi.OK
    torch_cuda.cuda.synchronize()
    assert out.untouched() and select_ctx.stats()["kernels_launched"] == launched


# ---- 6. the chain from host buffers ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coarse", [0, mc.COARSE])
def test_p_tree_merge_pu_frame_equals_the_pieces(oracle, torch_cuda, coarse):
    """the two-motion pair through the one-call form, and through its pieces queued on one stream: zero-centred (both merge stages at the search range) and
    centred (both at 64); the counters of the one-call form"""
    torch = torch_cuda
    cur, ref = mc.pictures()
    w, h, qp = mc.W, mc.H, mc.QP
    R = mc.CENTRED_RANGE if coarse else mc.RANGE
    MRG = mc.CENTRED_MERGE_RANGE if coarse else R
    c = capi.Context(w, h, 8, max_frames=2)
    n = c.num_ctus
    d_luma = to_dev(torch, np.stack([ref, cur]))
    cen = Guarded(torch, n * 16)
    found = [Guarded(torch, n * k * 16) for k in (85, 124, 384)]
    fine = [Guarded(torch, n * k * 16) for k in (85, 124, 384)]
    merge, shapes, dmin, dmax = Guarded(torch, n * 85 * 16), Guarded(torch, n * 85 * 16), Guarded(torch, n * 256), Guarded(torch, n * 256)
    mpu = {f: Guarded(torch, n * PER[f] * 16) for f in BOTH}
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
    c.motion_merge_device(p, 1, w, w * h, 2, fine[0].ptr, merge.ptr, stream=s, qp=qp, max_range=MRG)
    c.motion_merge_pu_device(p, 1, w, w * h, 2, fine[0].ptr, mpu["pu"].ptr, mpu["small"].ptr, stream=s, qp=qp, max_range=MRG)
    c.pu_shape_select_merge_device(fine[0].ptr, fine[1].ptr, fine[2].ptr, mpu["pu"].ptr, mpu["small"].ptr, 1, shapes.ptr, stream=s)
    c.p_tree_select_merge_device(shapes.ptr, merge.ptr, 1, dmin.ptr, dmax.ptr, None, stream=s)
    torch.cuda.synchronize()
    piece_launches = c.stats()["kernels_launched"] - launched
    pieces = dict(merge=merge.result(MDT, (n, 85)), shapes=shapes.result(SDT, (n, 85)), dmin=dmin.result(np.uint8, (n, 256)), dmax=dmax.result(np.uint8, (n, 256)))
    # the pieces against the restatements, on the pieces' own refined entries
    refined = [g.result(QDT, (n, k)) for g, k in zip(fine, (85, 124, 384))]
    flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
    emp = {f: mpr.expected(oracle, flat, 0, w, ref.astype(np.int64), w, h, 8, qp, refined[0], MRG, f) for f in BOTH}
    for f in BOTH:
        mpr.same(mpu[f].result(MDT, (n, PER[f])), emp[f], ("pieces", f, coarse))
    erec, _, emerged = mpr.select(refined[0][None], refined[1][None], refined[2][None], emp["pu"][None], emp["small"][None], w, h)
    sr.same(pieces["shapes"], erec[0], ("pieces", coarse))
    plain = sr.select(refined[0][None], refined[1][None], refined[2][None], w, h)[0][0]
    assert emerged.any() and (plain["cost_best"] != erec[0]["cost_best"]).any() and (plain["best"] != erec[0]["best"]).any()
    # the one-call form
    bc, org, stride = pel(cur)
    br, _, _ = pel(ref)
    before = c.stats()
    lo, hi, sh, me = c.p_tree_merge_pu_frame(bc, br, org, stride, qp=qp, search_range=R, coarse_range=coarse, with_shapes=True, with_merge=True)
    after = c.stats()
    assert lo.tobytes() == pieces["dmin"].tobytes() and hi.tobytes() == pieces["dmax"].tobytes()
    assert sh.tobytes() == pieces["shapes"].tobytes() and me.tobytes() == pieces["merge"].tobytes()
    assert after["bytes_h2d"] - before["bytes_h2d"] == w * h * 4 and after["bytes_d2h"] - before["bytes_d2h"] == n * (512 + 2 * 85 * 16)
    assert after["kernels_launched"] - before["kernels_launched"] == piece_launches
    before = after
    lo2, hi2 = c.p_tree_merge_pu_frame(bc, br, org, stride, qp=qp, search_range=R, coarse_range=coarse)
    assert lo2.tobytes() == lo.tobytes() and hi2.tobytes() == hi.tobytes() and c.stats()["bytes_d2h"] - before["bytes_d2h"] == n * 512
    # fhevc_p_tree_merge_frame is what it was: the plain selection's records, one launch fewer
    before = c.stats()
    _, _, sh0, me0 = c.p_tree_merge_frame(bc, br, org, stride, qp=qp, search_range=R, coarse_range=coarse, with_shapes=True, with_merge=True)
    assert c.stats()["kernels_launched"] - before["kernels_launched"] == piece_launches - 1
    sr.same(sh0, plain, "merge_frame")
    assert me0.tobytes() == me.tobytes()
    # the frame form rejects what fhevc_p_tree_merge_frame rejects, before anything is launched
    launched = c.stats()["kernels_launched"]
    for change in (dict(search_range=9, coarse_range=1), dict(coarse_range=15), dict(search_range=65), dict(qp=52)):
        with pytest.raises(capi.FastHevcError):
            c.p_tree_merge_pu_frame(bc, br, org, stride, **dict(dict(qp=qp, search_range=R, coarse_range=coarse), **change))
    assert c.stats()["kernels_launched"] == launched
    c.close()
