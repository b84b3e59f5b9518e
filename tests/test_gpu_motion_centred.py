"""Config 4 (P slices), the chain around a predictor on the MI355X: the coarse motion centres, fhevc_motion_centres* (k_motion_coarse.hip); the integer
searches around them, fhevc_motion_search_pu_centred* (the centred instantiations of k_motion_pu.hip and k_motion_pu_small.hip); their quarter-sample
refinements, fhevc_motion_refine_pu_centred* (those of k_motion_refine.hip and k_motion_refine_pu.hip); and the whole chain into
fhevc_pu_shape_select_device.  Against the numpy restatements (tests/motion_centred_ref.py, pinned without a GPU by test_motion_centred_ref.py), against what
the reference itself returned (tests/golden/ref_motion_centred.npz: the entries whose reads stay inside the picture, counted) and, with zero centres, against
fhevc_motion_search_pu_wide_device / fhevc_motion_refine_pu_wide_device.  Bit for bit, every field, markers included."""
import numpy as np
import pytest

import motion_centred_ref as cr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, Guarded, clip_planes, pel, pel_batch, same, to_dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

DT = capi.MOTION_DTYPE
MARKER = cr.MARKER


def run_dev(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, qp, Rc, rows=None, stream=None, d_luma=None, out_skew=0):
    """one call over a device batch -> [nf - 1, band CTUs]; the guards around the output are checked.  out_skew: bytes added to the output pointer"""
    rows_ = rows or (0, ctx.ctus_y)
    n = (rows_[1] - rows_[0]) * ctx.ctus_x
    d_luma = to_dev(torch, flat) if d_luma is None else d_luma
    g = Guarded(torch, max((nf - 1) * n * 16, 16) + out_skew)
    torch.cuda.synchronize()
    ctx.motion_centres_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, g.ptr + out_skew, rows=rows, stream=stream, qp=qp,
                              coarse_range=Rc)
    torch.cuda.synchronize()
    h = g.t.cpu().numpy()
    assert (h[:g.GUARD + out_skew] == CANARY).all() and (h[g.GUARD + g.n:] == CANARY).all(), "bytes around the output were written"
    return h[g.GUARD + out_skew:g.GUARD + g.n].copy().view(DT).reshape(nf - 1, n)


def expected(pics, bd, qp, Rc):
    """[len(pics) - 1, numCtus]: picture f searched in picture f - 1"""
    sl = cr.sqrt_lambda(qp)
    return np.stack([cr.centres(pics[f], pics[f - 1], bd, sl, Rc) for f in range(1, len(pics))])


def moving_pictures(W, H, bd, nf, seed):
    """nf pictures cut from one texture at positions that move by another vector per picture, plus noise so that no distortion is zero"""
    rng = np.random.default_rng(seed)
    big = cr.texture(W, H, bd, seed)
    pos = [(64, 64)]
    for v in ((12, -8), (-28, 20), (4, 36))[:nf - 1]:
        pos.append((pos[-1][0] + v[0], pos[-1][1] + v[1]))
    return [np.clip(big[y:y + H, x:x + W] + rng.integers(-(3 << (bd - 8)), (3 << (bd - 8)) + 1, size=(H, W)), 0, (1 << bd) - 1) for x, y in pos]


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(176, 144), (104, 88)])
@pytest.mark.parametrize("bd,qp", [(8, 30), (10, 22), (12, 41)])
def test_int16_planes_vs_restatement(torch_cuda, W, H, bd, qp):
    """three pictures in TComPicYuv's layout (margins, an origin and a stride that are no multiples of 8 at 104 x 88); 104 x 88 is ragged both ways:
    the last CTU column owns 10 cell columns, the last row 6 cell rows"""
    torch = torch_cuda
    pics = moving_pictures(W, H, bd, 3, seed=bd + W)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=3)
    for Rc in (1, 7, 14):
        got = run_dev(torch, ctx, flat, org, stride, fs, 3, 2, qp, Rc, d_luma=d_luma)
        same(got, expected(pics, bd, qp, Rc), (W, H, bd, Rc))
        assert (got["cost_best"] != MARKER).all()
    ctx.close()


@pytest.mark.parametrize("W,H,Rc", [(176, 144, 14), (104, 88, 7), (104, 88, 1), (66, 70, 3)])
def test_uint8_planes_vs_restatement_and_equal_int16(torch_cuda, W, H, Rc):
    """uint8 planes without margins (66 x 70: the second CTU column is 2 samples wide and owns no cell -- the marker --, the second row owns one cell
    row), and the same pictures as int16 planes: the same bytes"""
    torch = torch_cuda
    qp = 27 + Rc
    pics = moving_pictures(W, H, 8, 3, seed=W + Rc)
    ctx = capi.Context(W, H, 8, max_frames=3)
    got = run_dev(torch, ctx, np.stack(pics).astype(np.uint8), 0, W, W * H, 3, 1, qp, Rc)
    exp = expected(pics, 8, qp, Rc)
    same(got, exp, (W, H, Rc))
    assert run_dev(torch, ctx, np.stack(pics).astype(np.int16), 0, W, W * H, 3, 2, qp, Rc).tobytes() == got.tobytes()
    if W == 66:
        assert (got[:, 1::2]["cost_best"] == MARKER).all() and (got[:, 0::2]["cost_best"] != MARKER).all() and (got[:, 1::2]["mvx"] == 0).all()
    ctx.close()


@pytest.mark.parametrize("bd,qp,v", [(8, 32, (20, -12)), (10, 27, (-24, 4)), (12, 37, (56, -56)), (8, 51, (-56, 56))])
def test_constructed_pans_are_found_exactly_on_interior_ctus(torch_cuda, bd, qp, v):
    torch = torch_cuda
    W, H = 320, 256
    cur, ref = cr.panned_pair(W, H, bd, seed=bd + qp, vx=v[0], vy=v[1])
    (rb, org, stride), (cb, _, _) = pel(ref), pel(cur)
    ctx = capi.Context(W, H, bd)
    got = ctx.motion_centres(cb, rb, org, stride, qp=qp, coarse_range=14)      # the host form
    same(got, cr.centres(cur, ref, bd, cr.sqrt_lambda(qp), 14), (bd, v))
    inner = got.reshape(4, 5)[1:3, 1:4]
    assert (inner["mvx"] == v[0]).all() and (inner["mvy"] == v[1]).all() and (inner["satd_best"] == 0).all() and (inner["satd_zero"] > inner["cost_best"]).all()
    # the device form over the same pair writes the same bytes
    flat, org2, stride2, fs = pel_batch([ref, cur])
    assert run_dev(torch, ctx, flat, org2, stride2, fs, 2, 2, qp, 14)[0].tobytes() == got.tobytes()
    ctx.close()


def test_flat_content_lands_on_zero(torch_cuda):
    W, H, bd = 176, 144, 10
    flat = np.full((H, W), 1021, np.int64)
    (b, org, stride) = pel(flat)
    ctx = capi.Context(W, H, bd)
    got = ctx.motion_centres(b, b, org, stride, qp=33, coarse_range=14)
    assert (got["mvx"] == 0).all() and (got["mvy"] == 0).all() and (got["satd_zero"] == 0).all() and (got["satd_best"] == 0).all()
    assert (got["cost_best"] == cr.bit_cost(2, cr.sqrt_lambda(33))).all()
    ctx.close()


# ---- 2. layouts ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sample_bytes,bd", [(2, 10), (1, 8)])
def test_planes_between_poison_odd_origin_and_stride_a_band_and_a_skewed_output(torch_cuda, sample_bytes, bd):
    """every sample outside the pictures holds the largest value of the plane's type, origin and stride are odd (no 16-byte row loads), the frames lie
    an odd number of samples apart; the whole picture, then each band of CTU rows; the output 4 bytes off a 16-byte boundary"""
    torch = torch_cuda
    W, H, NF, qp, Rc = 104, 152, 3, 36, 5
    pics = moving_pictures(W, H, bd, NF, seed=77 + bd)
    stride, top, left = W + 13, 3, 7
    fs = stride * (H + 5) + 1
    dt = np.int16 if sample_bytes == 2 else np.uint8
    flat = np.full(NF * fs + 64, np.iinfo(dt).max, dt)
    org = top * stride + left
    for f, p in enumerate(pics):
        v = flat[f * fs + org:f * fs + org + H * stride].reshape(H, stride) if f * fs + org + H * stride <= flat.size else None
        assert v is not None
        v[:, :W] = p
    ctx = capi.Context(W, H, bd, max_frames=NF)
    exp = expected(pics, bd, qp, Rc)
    d_luma = to_dev(torch, flat)
    got = run_dev(torch, ctx, flat, org, stride, fs, NF, sample_bytes, qp, Rc, d_luma=d_luma, out_skew=4)
    same(got, exp, "whole")
    cw = ctx.ctus_x
    for rows in ((0, 1), (1, 3), (2, 3)):
        band = run_dev(torch, ctx, flat, org, stride, fs, NF, sample_bytes, qp, Rc, rows=rows, d_luma=d_luma)
        same(band, exp[:, rows[0] * cw:rows[1] * cw], rows)
    # an empty band writes nothing
    g = Guarded(torch, 64)
    ctx.motion_centres_device(d_luma.data_ptr() + sample_bytes * org, sample_bytes, stride, fs, NF, g.ptr, rows=(2, 2), qp=qp, coarse_range=Rc)
    torch.cuda.synchronize()
    assert g.untouched()
    ctx.close()


def test_more_ctus_than_the_grid(torch_cuda):
    """the persistent grid holds at most eight workgroups per CU: 17 pairs of 1024 x 576 are 2 448 CTUs, more than 8 x 256"""
    torch = torch_cuda
    W, H, NF, qp, Rc = 1024, 576, 18, 31, 2
    rng = np.random.default_rng(3)
    big = cr.texture(W + 4 * NF, H + 4 * NF, 8, 11, margin=0)
    pics = [np.clip(big[4 * f:4 * f + H, 4 * (NF - f):4 * (NF - f) + W] + rng.integers(-2, 3, size=(H, W)), 0, 255) for f in range(NF)]
    ctx = capi.Context(W, H, 8, max_frames=NF)
    assert (NF - 1) * ctx.num_ctus > 8 * 256
    got = run_dev(torch, ctx, np.stack(pics).astype(np.uint8), 0, W, W * H, NF, 1, qp, Rc)
    same(got, expected(pics, 8, qp, Rc))
    inner = got.reshape(NF - 1, ctx.ctus_y, ctx.ctus_x)[:, 1:-1, 1:-1]
    assert (inner["mvx"] == -4).all() and (inner["mvy"] == 4).all()
    ctx.close()


# ---- 3. streams, timing, rejected calls ---------------------------------------------------------------------------------------------------------------------

def test_two_streams_with_different_qps_and_ranges(torch_cuda):
    torch = torch_cuda
    W, H, bd, NF = 176, 144, 8, 3
    pics = moving_pictures(W, H, bd, NF, seed=5)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    n = ctx.num_ctus
    cases = [(12, 14), (45, 3)]
    streams = [torch.cuda.Stream() for _ in cases]
    outs = [[Guarded(torch, (NF - 1) * n * 16) for _ in range(4)] for _ in cases]
    torch.cuda.synchronize()
    for rep in range(4):      # interleaved: neither stream waits for the other, nothing is synchronised in between
        for (qp, Rc), st, o in zip(cases, streams, outs):
            ctx.motion_centres_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, o[rep].ptr, stream=st.cuda_stream, qp=qp, coarse_range=Rc)
    torch.cuda.synchronize()
    for (qp, Rc), o in zip(cases, outs):
        exp = expected(pics, bd, qp, Rc)
        for g in o:
            same(g.result((NF - 1, n)), exp, (qp, Rc))
    ctx.close()


def test_slot_15_counts_one_launch_per_call(torch_cuda):
    torch = torch_cuda
    W, H = 104, 88
    pics = moving_pictures(W, H, 8, 2, seed=9)
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8))
    ctx = capi.Context(W, H, 8, max_frames=2)
    out = Guarded(torch, ctx.num_ctus * 16)
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(15, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls in (1, 2):
        ctx.motion_centres_device(d_luma.data_ptr(), 1, W, W * H, 2, out.ptr, qp=30, coarse_range=4)
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(15)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (4, 8, 11, 12, 13))
    ctx.enable_kernel_timing(False)
    for bad in (14, 16):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(bad)
    ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H = 104, 88
    lib = capi.load_library()
    d8 = to_dev(torch, np.zeros((2, H, W), np.uint8))
    out = Guarded(torch, 4 * 16)
    for bd in (8, 10):
        ctx = capi.Context(W, H, bd, max_frames=2)
        good = dict(d_luma=d8.data_ptr(), sb=1 if bd == 8 else 2, stride=W, fs=W * H, nf=2, rb=0, re=2, qp=30, rc=14, out=out.ptr)
        bad = [dict(d_luma=None), dict(out=None), dict(nf=1), dict(qp=-1), dict(qp=52), dict(rc=0), dict(rc=15), dict(stride=W - 1), dict(rb=-1), dict(re=3),
               dict(rb=2, re=1), dict(sb=4), dict(fs=W * H - W - 1)]
        if bd == 10:
            bad.append(dict(sb=1))       # uint8 planes on a context above 8 bit
        for change in bad:
            a = dict(good, **change)
            rc = lib.fhevc_motion_centres_device(ctx.h, a["d_luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["rc"], a["out"], None)
            assert rc == capi.E_INVALID, (bd, change)
            assert lib.fhevc_last_error(ctx.h), change
        torch.cuda.synchronize()
        assert out.untouched()
        ctx.close()


# ---- 4. the integer searches around a centre (fhevc_motion_search_pu_centred*) --------------------------------------------------------------------------------

FAMS = cr.FAMS
PER = {"nodes": capi.NODES_PER_CTU, "pu": capi.PUS_PER_CTU, "small": capi.PUS_SMALL_PER_CTU}


def search_dev(torch, ctx, d_luma, origin, stride, fstride, nf, sample_bytes, qp, R, centres, rows=None, stream=None, fams=FAMS, centre_skew=0):
    """one centred call -> {family: [nf - 1, band CTUs, entries]}; centres: [nf - 1, band CTUs] records, uploaded centre_skew bytes off a 16-byte boundary;
    the guards are checked and the outputs of the families NOT asked for stay untouched"""
    rows_ = rows or (0, ctx.ctus_y)
    n = (rows_[1] - rows_[0]) * ctx.ctus_x
    assert centres.shape == (nf - 1, n)
    raw = np.full(centres.size * 16 + 16, CANARY, np.uint8)
    raw[centre_skew:centre_skew + centres.size * 16] = np.ascontiguousarray(centres).view(np.uint8).reshape(-1)
    d_cen = to_dev(torch, raw)
    g = {f: Guarded(torch, max((nf - 1) * n * PER[f] * 16, 16)) for f in FAMS}
    torch.cuda.synchronize()
    ctx.motion_search_pu_centred_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, d_cen.data_ptr() + centre_skew,
                                        *(g[f].ptr if f in fams else None for f in FAMS), rows=rows, stream=stream, qp=qp, search_range=R)
    torch.cuda.synchronize()
    assert all(g[f].untouched() for f in FAMS if f not in fams)
    return {f: g[f].result((nf - 1, n, PER[f])) for f in fams}


def expected_search(oracle, pics, bd, qp, R, centres):
    """{family: [len(pics) - 1, numCtus, entries]}; centres [len(pics) - 1, numCtus]"""
    per = [cr.centred_search(oracle, pics[f], pics[f - 1], bd, qp, R, centres[f - 1]) for f in range(1, len(pics))]
    return {f: np.stack([p[f] for p in per]) for f in FAMS}


def same_fams(got, exp, what=""):
    for f in got:
        same(got[f], exp[f], (what, f))


# nine CTUs of 176 x 144: the window pushed wholly outside the picture at the first and the last CTU, every column residue mod 8 (-56, 5, -22, 23, 12, -3, -31, 9,
# 56 are 0, 5, 2, 7, 4, 5, 1, 1, 0; the second picture pair adds 3 and 6), different centres per CTU
CENTRES_9 = [[(-56, -56), (5, -17), (-22, 40), (23, 0), (12, -12), (-3, 56), (-31, -8), (9, 33), (56, 56)],
             [(3, 1), (-2, 7), (6, -5), (0, 0), (-56, 56), (56, -56), (14, 14), (-21, 2), (43, -40)]]
CENTRES_4 = [[(-56, -56), (17, -6), (-9, 30), (56, 56)], [(2, -3), (-12, 1), (7, 7), (-20, -44)]]


@pytest.mark.parametrize("W,H,cen", [(176, 144, CENTRES_9), (104, 88, CENTRES_4)])
@pytest.mark.parametrize("bd,qp", [(8, 30), (10, 22), (12, 41)])
def test_centred_search_vs_restatement_on_every_entry(oracle, torch_cuda, W, H, cen, bd, qp):
    torch = torch_cuda
    pics = moving_pictures(W, H, bd, 3, seed=2 * bd + W)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=3)
    centres = np.stack([cr.make_centres(c) for c in cen])
    assert W != 176 or all({(x - R) % 8 for c in cen for x, _ in c} == set(range(8)) for R in (1, 5, 8))      # every 8-sample phase of the window's first column
    for R in (1, 5, 8):
        got = search_dev(torch, ctx, d_luma, org, stride, fs, 3, 2, qp, R, centres)
        exp = expected_search(oracle, pics, bd, qp, R, centres)
        same_fams(got, exp, (W, bd, R))
        valid = {f: exp[f]["cost_best"] != MARKER for f in FAMS}
        for f in FAMS:     # absolute vectors inside the window around the centre
            dx = got[f]["mvx"] - centres["mvx"][..., None]
            dy = got[f]["mvy"] - centres["mvy"][..., None]
            assert (np.abs(dx)[valid[f]] <= R).all() and (np.abs(dy)[valid[f]] <= R).all()
        if R == 5:         # each family alone writes the same bytes and leaves the other outputs alone
            for f in FAMS:
                assert search_dev(torch, ctx, d_luma, org, stride, fs, 3, 2, qp, R, centres, fams=(f,))[f].tobytes() == got[f].tobytes(), f
    ctx.close()


@pytest.mark.parametrize("bd,sample_bytes", [(8, 1), (8, 2), (10, 2), (12, 2)])
def test_zero_centres_write_the_bytes_of_the_wide_search(torch_cuda, bd, sample_bytes):
    torch = torch_cuda
    W, H, NF, qp = 176, 144, 3, 28
    pics = moving_pictures(W, H, bd, NF, seed=31 + bd)
    flat = np.stack(pics).astype(np.uint8 if sample_bytes == 1 else np.int16)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    n = ctx.num_ctus
    zero = np.stack([cr.make_centres([(0, 0)] * n)] * (NF - 1))
    for R in (1, 5, 8):
        got = search_dev(torch, ctx, d_luma, 0, W, W * H, NF, sample_bytes, qp, R, zero)
        g = {f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}
        torch.cuda.synchronize()
        ctx.motion_search_pu_wide_device(d_luma.data_ptr(), sample_bytes, W, W * H, NF, g["nodes"].ptr, g["pu"].ptr, g["small"].ptr, qp=qp, search_range=R)
        torch.cuda.synchronize()
        for f in FAMS:
            assert g[f].result((NF - 1, n, PER[f])).tobytes() == got[f].tobytes(), (bd, R, f)
    ctx.close()


def test_an_out_of_range_centre_marks_exactly_its_ctu(oracle, torch_cuda):
    torch = torch_cuda
    W, H, bd, qp, R = 176, 144, 8, 33, 8
    pics = moving_pictures(W, H, bd, 2, seed=4)
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8))
    ctx = capi.Context(W, H, bd, max_frames=2)
    good = [(5, -6)] * 9
    ref = search_dev(torch, ctx, d_luma, 0, W, W * H, 2, 1, qp, R, cr.make_centres(good)[None])
    for bad in ((57, 0), (0, -57), (-32768, 32767), (-57, 57)):
        cen = list(good)
        cen[4] = bad
        got = search_dev(torch, ctx, d_luma, 0, W, W * H, 2, 1, qp, R, cr.make_centres(cen)[None])
        for f in FAMS:
            a = got[f][0]
            assert (a[4]["satd_zero"] == MARKER).all() and (a[4]["satd_best"] == MARKER).all() and (a[4]["cost_best"] == MARKER).all()
            assert (a[4]["mvx"] == 0).all() and (a[4]["mvy"] == 0).all()
            others = [c for c in range(9) if c != 4]
            assert a[others].tobytes() == ref[f][0][others].tobytes(), (bad, f)
    same_fams(ref, expected_search(oracle, pics, bd, qp, R, cr.make_centres(good)[None]))
    ctx.close()


@pytest.mark.parametrize("sample_bytes,bd", [(2, 10), (1, 8)])
def test_centred_search_layouts(oracle, torch_cuda, sample_bytes, bd):
    """planes between poison, odd origin and stride, a band, centres 4 bytes off a 16-byte boundary"""
    torch = torch_cuda
    W, H, NF, qp, R = 104, 152, 3, 36, 8
    pics = moving_pictures(W, H, bd, NF, seed=70 + bd)
    stride, top, left = W + 13, 3, 7
    fs = stride * (H + 5) + 1
    dt = np.int16 if sample_bytes == 2 else np.uint8
    flat = np.full(NF * fs + 64, np.iinfo(dt).max, dt)
    org = top * stride + left
    for f, p in enumerate(pics):
        flat[f * fs + org:f * fs + org + H * stride].reshape(H, stride)[:, :W] = p
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    rng = np.random.default_rng(bd)
    centres = np.stack([cr.make_centres([tuple(int(v) for v in rng.integers(-56, 57, size=2)) for _ in range(6)]) for _ in range(NF - 1)])
    exp = expected_search(oracle, pics, bd, qp, R, centres)
    same_fams(search_dev(torch, ctx, d_luma, org, stride, fs, NF, sample_bytes, qp, R, centres, centre_skew=4), exp, "whole")
    for rows in ((0, 1), (1, 3)):
        sl = slice(rows[0] * 2, rows[1] * 2)
        band = search_dev(torch, ctx, d_luma, org, stride, fs, NF, sample_bytes, qp, R, np.ascontiguousarray(centres[:, sl]), rows=rows, centre_skew=12)
        same_fams(band, {f: exp[f][:, sl] for f in FAMS}, rows)
    ctx.close()


def test_centred_search_more_ctus_than_the_grid(oracle, torch_cuda):
    """9 pairs of 1024 x 576 are 1 296 CTUs: more than the four workgroups per CU of the small-PU kernel's grid; every 41st CTU against the restatement, all of
    them against the wide search where the centre is zero"""
    torch = torch_cuda
    W, H, NF, qp, R = 1024, 576, 10, 31, 3
    rng = np.random.default_rng(3)
    big = cr.texture(W + 4 * NF, H + 4 * NF, 8, 12, margin=0)
    pics = [np.clip(big[4 * f:4 * f + H, 4 * (NF - f):4 * (NF - f) + W] + rng.integers(-2, 3, size=(H, W)), 0, 255) for f in range(NF)]
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    assert (NF - 1) * n > 4 * 256
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8))
    centres = np.stack([cr.make_centres([(-4, 4) if (c + p) % 3 else (0, 0) for c in range(n)]) for p in range(NF - 1)])
    got = search_dev(torch, ctx, d_luma, 0, W, W * H, NF, 1, qp, R, centres)
    for p in range(NF - 1):
        ctus = [c for c in range(n) if (c + 7 * p) % 41 == 0]
        exp = cr.centred_search(oracle, pics[p + 1], pics[p], 8, qp, R, centres[p], ctus=ctus)
        for f in FAMS:
            same(got[f][p][ctus], exp[f][ctus], (p, f))
    g = {f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}
    ctx.motion_search_pu_wide_device(d_luma.data_ptr(), 1, W, W * H, NF, g["nodes"].ptr, g["pu"].ptr, g["small"].ptr, qp=qp, search_range=R)
    torch.cuda.synchronize()
    zero = (centres["mvx"] == 0)
    for f in FAMS:
        assert g[f].result((NF - 1, n, PER[f]))[zero].tobytes() == got[f][zero].tobytes(), f
    ctx.close()


def test_chain_centres_then_search_on_one_stream_and_two_chains_on_two_streams(oracle, torch_cuda):
    """centres -> centred search on one stream with no host synchronisation in between, two such chains with different QPs and ranges in flight together"""
    torch = torch_cuda
    W, H, bd, NF = 176, 144, 8, 3
    pics = moving_pictures(W, H, bd, NF, seed=15)
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8))
    ctx = capi.Context(W, H, bd, max_frames=NF)
    n = ctx.num_ctus
    cases = [(24, 14, 8), (40, 5, 3)]      # QP, coarse range, search range
    streams = [torch.cuda.Stream() for _ in cases]
    cen = [Guarded(torch, (NF - 1) * n * 16) for _ in cases]
    outs = [{f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS} for _ in cases]
    torch.cuda.synchronize()
    for (qp, Rc, R), st, c, o in zip(cases, streams, cen, outs):
        ctx.motion_centres_device(d_luma.data_ptr(), 1, W, W * H, NF, c.ptr, stream=st.cuda_stream, qp=qp, coarse_range=Rc)
    for (qp, Rc, R), st, c, o in zip(cases, streams, cen, outs):
        ctx.motion_search_pu_centred_device(d_luma.data_ptr(), 1, W, W * H, NF, c.ptr, o["nodes"].ptr, o["pu"].ptr, o["small"].ptr, stream=st.cuda_stream, qp=qp, search_range=R)
    torch.cuda.synchronize()
    for (qp, Rc, R), c, o in zip(cases, cen, outs):
        centres = expected(pics, bd, qp, Rc)
        same(c.result((NF - 1, n)), centres, (qp, "centres"))
        exp = expected_search(oracle, pics, bd, qp, R, centres)
        same_fams({f: o[f].result((NF - 1, n, PER[f])) for f in FAMS}, exp, (qp, R))
    # the centres of this content are not all zero: the chain really searched around them
    assert (expected(pics, bd, 24, 14)["mvx"] != 0).any()
    ctx.close()


def test_centred_search_host_form_timing_and_rejected_calls(oracle, torch_cuda):
    torch = torch_cuda
    W, H, bd, qp, R = 104, 88, 10, 27, 5
    pics = moving_pictures(W, H, bd, 2, seed=21)
    (rb, org, stride), (cb, _, _) = pel(pics[0]), pel(pics[1])
    ctx = capi.Context(W, H, bd, max_frames=2)
    centres = cr.make_centres(CENTRES_4[0])
    exp = cr.centred_search(oracle, pics[1], pics[0], bd, qp, R, centres)
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(15, reset=True)
    got = dict(zip(FAMS, ctx.motion_search_pu_centred(cb, rb, centres, org, stride, qp=qp, search_range=R)))
    same_fams(got, exp, "host form")
    assert ctx.kernel_timing(15)[1] == 2           # one launch for nodes and PUs, one for the small PUs
    alone = ctx.motion_search_pu_centred(cb, rb, centres, org, stride, qp=qp, search_range=R, nodes=True, pus=False, pus_small=False)
    assert alone[1] is None and alone[2] is None and alone[0].tobytes() == got["nodes"].tobytes()
    assert ctx.kernel_timing(15)[1] == 3
    ctx.enable_kernel_timing(False)
    # rejected calls write nothing
    lib = capi.load_library()
    d = to_dev(torch, np.zeros((2, H, W), np.int16))
    cen = to_dev(torch, centres)
    out = [Guarded(torch, 4 * PER[f] * 16) for f in FAMS]
    good = dict(d_luma=d.data_ptr(), sb=2, stride=W, fs=W * H, nf=2, rb=0, re=2, qp=30, R=8, cen=cen.data_ptr(), o0=out[0].ptr, o1=out[1].ptr, o2=out[2].ptr)
    for change in (dict(d_luma=None), dict(cen=None), dict(o0=None, o1=None, o2=None), dict(nf=1), dict(qp=-1), dict(qp=52), dict(R=0), dict(R=9), dict(stride=W - 1),
                   dict(rb=-1), dict(re=3), dict(rb=2, re=1), dict(sb=1), dict(sb=3), dict(fs=W * H - W - 1)):
        a = dict(good, **change)
        rc = lib.fhevc_motion_search_pu_centred_device(ctx.h, a["d_luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["cen"], a["o0"], a["o1"],
                                                       a["o2"], None)
        assert rc == capi.E_INVALID, change
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out)
    ctx.close()


# ---- 5. the quarter-sample refinements around a centre (fhevc_motion_refine_pu_centred*) ------------------------------------------------------------------------

QDT = capi.MOTION_QPEL_DTYPE


def refine_dev(torch, ctx, d_luma, origin, stride, fstride, nf, sample_bytes, qp, max_range, centres, ins, rows=None, stream=None, fams=FAMS, centre_skew=0):
    """one centred refinement -> {family: [nf - 1, band CTUs, entries]} of MOTION_QPEL_DTYPE; ins: {family: records}; guards checked, the outputs of the families
    not asked for stay untouched"""
    rows_ = rows or (0, ctx.ctus_y)
    n = (rows_[1] - rows_[0]) * ctx.ctus_x
    raw = np.full(centres.size * 16 + 16, CANARY, np.uint8)
    raw[centre_skew:centre_skew + centres.size * 16] = np.ascontiguousarray(centres).view(np.uint8).reshape(-1)
    d_cen = to_dev(torch, raw)
    d_in = {f: to_dev(torch, ins[f]) for f in fams}
    g = {f: Guarded(torch, max((nf - 1) * n * PER[f] * 16, 16)) for f in FAMS}
    args = []
    for f in FAMS:
        args += [d_in[f].data_ptr(), g[f].ptr] if f in fams else [None, None]
    torch.cuda.synchronize()
    ctx.motion_refine_pu_centred_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, d_cen.data_ptr() + centre_skew, *args,
                                        rows=rows, stream=stream, qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    assert all(g[f].untouched() for f in FAMS if f not in fams)
    return {f: g[f].result((nf - 1, n, PER[f])).view(QDT) for f in fams}


def same_q(got, exp, what=""):
    for f in got:
        for k in QDT.names:
            bad = got[f][k] != exp[f][k]
            assert not bad.any(), (what, f, k, np.argwhere(bad)[:5], got[f][k][bad][:5], exp[f][k][bad][:5])


def with_random_vectors(recs, centres, R, seed):
    """every 7th entry gets a random vector inside the window around its CTU's centre, every 31st one just outside it (the marker)"""
    rng = np.random.default_rng(seed)
    out = {}
    for f, a in recs.items():
        a = a.copy()
        idx = np.arange(a.shape[-1])
        for name, c in (("mvx", centres["mvx"]), ("mvy", centres["mvy"])):
            rnd = c[..., None] + rng.integers(-R, R + 1, size=a.shape)
            v = np.where(idx % 7 == 0, rnd, a[name])
            a[name] = np.where(idx % 31 == 5, c[..., None] + (R + 1 if name == "mvx" else -R - 1), v)
        out[f] = a
    return out


@pytest.mark.parametrize("W,H,cen,bd,qp,R", [(176, 144, CENTRES_9, 8, 30, 1), (176, 144, CENTRES_9, 10, 22, 5), (176, 144, CENTRES_9, 12, 41, 8), (104, 88, CENTRES_4, 8, 35, 8)])
def test_centred_refinement_vs_restatement_on_every_entry(oracle, torch_cuda, W, H, cen, bd, qp, R):
    """around the centred search's own vectors, every 7th entry a random vector of the window, every 31st outside it; windows on every column residue, pushed
    outside the picture at two corners, ragged CTUs; all three families together and each alone"""
    torch = torch_cuda
    pics = moving_pictures(W, H, bd, 2, seed=3 * bd + W)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=2)
    centres = np.stack([cr.make_centres(cen[0])])
    ints = with_random_vectors(search_dev(torch, ctx, d_luma, org, stride, fs, 2, 2, qp, R, centres), centres, R, seed=R)
    got = refine_dev(torch, ctx, d_luma, org, stride, fs, 2, 2, qp, R, centres, ints, centre_skew=8)
    exp = cr.centred_refine(oracle, pics[1], pics[0], bd, qp, R, centres[0], {f: ints[f][0] for f in FAMS})
    same_q({f: got[f][0] for f in FAMS}, exp, (W, bd, R))
    marked = {f: int((exp[f]["cost_best"] == MARKER).sum()) for f in FAMS}
    assert all(marked[f] >= PER[f] // 31 for f in FAMS)       # the vectors outside the window, and the entries whose node leaves the picture
    for f in FAMS:
        assert refine_dev(torch, ctx, d_luma, org, stride, fs, 2, 2, qp, R, centres, ints, fams=(f,))[f].tobytes() == got[f].tobytes(), f
    ctx.close()


@pytest.mark.parametrize("bd,sample_bytes", [(8, 1), (10, 2), (12, 2)])
def test_zero_centres_write_the_bytes_of_the_wide_refinement(torch_cuda, bd, sample_bytes):
    torch = torch_cuda
    W, H, NF, qp = 176, 144, 3, 28
    pics = moving_pictures(W, H, bd, NF, seed=41 + bd)
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8 if sample_bytes == 1 else np.int16))
    ctx = capi.Context(W, H, bd, max_frames=NF)
    n = ctx.num_ctus
    zero = np.stack([cr.make_centres([(0, 0)] * n)] * (NF - 1))
    for R in (1, 5, 8):
        ints = with_random_vectors(search_dev(torch, ctx, d_luma, 0, W, W * H, NF, sample_bytes, qp, R, zero), zero, R, seed=bd + R)
        got = refine_dev(torch, ctx, d_luma, 0, W, W * H, NF, sample_bytes, qp, R, zero, ints)
        d_in = {f: to_dev(torch, ints[f]) for f in FAMS}
        g = {f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}
        torch.cuda.synchronize()
        ctx.motion_refine_pu_wide_device(d_luma.data_ptr(), sample_bytes, W, W * H, NF, d_in["nodes"].data_ptr(), g["nodes"].ptr, d_in["pu"].data_ptr(), g["pu"].ptr,
                                         d_in["small"].data_ptr(), g["small"].ptr, qp=qp, max_range=R)
        torch.cuda.synchronize()
        for f in FAMS:
            assert g[f].result((NF - 1, n, PER[f])).tobytes() == got[f].tobytes(), (bd, R, f)
    ctx.close()


def test_refinement_an_out_of_range_centre_marks_exactly_its_ctu_and_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H, bd, qp, R = 176, 144, 8, 33, 8
    pics = moving_pictures(W, H, bd, 2, seed=4)
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8))
    ctx = capi.Context(W, H, bd, max_frames=2)
    good = cr.make_centres([(5, -6)] * 9)[None]
    ints = search_dev(torch, ctx, d_luma, 0, W, W * H, 2, 1, qp, R, good)
    ref = refine_dev(torch, ctx, d_luma, 0, W, W * H, 2, 1, qp, R, good, ints)
    for bad in ((57, 0), (0, -57)):
        cen = good.copy()
        cen["mvx"][0, 4], cen["mvy"][0, 4] = bad
        got = refine_dev(torch, ctx, d_luma, 0, W, W * H, 2, 1, qp, R, cen, ints)
        for f in FAMS:
            a = got[f][0]
            assert (a[4]["satd_int"] == MARKER).all() and (a[4]["satd_best"] == MARKER).all() and (a[4]["cost_best"] == MARKER).all() and (a[4]["mvx"] == 0).all()
            others = [c for c in range(9) if c != 4]
            assert a[others].tobytes() == ref[f][0][others].tobytes(), (bad, f)
    lib = capi.load_library()
    d_in = {f: to_dev(torch, ints[f]) for f in FAMS}
    cen = to_dev(torch, good)
    out = {f: Guarded(torch, 9 * PER[f] * 16) for f in FAMS}
    base = dict(d_luma=d_luma.data_ptr(), sb=1, stride=W, fs=W * H, nf=2, rb=0, re=3, qp=30, R=8, cen=cen.data_ptr(), i0=d_in["nodes"].data_ptr(), o0=out["nodes"].ptr,
                i1=d_in["pu"].data_ptr(), o1=out["pu"].ptr, i2=d_in["small"].data_ptr(), o2=out["small"].ptr)
    for change in (dict(d_luma=None), dict(cen=None), dict(i0=None, o0=None, i1=None, o1=None, i2=None, o2=None), dict(i1=None), dict(o2=None), dict(nf=1), dict(qp=52),
                   dict(R=0), dict(R=9), dict(stride=W - 1), dict(re=4), dict(sb=3)):
        a = dict(base, **change)
        rc = lib.fhevc_motion_refine_pu_centred_device(ctx.h, a["d_luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["cen"], a["i0"], a["o0"],
                                                       a["i1"], a["o1"], a["i2"], a["o2"], None)
        assert rc == capi.E_INVALID, change
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out.values())
    ctx.close()


def test_whole_chain_on_one_stream_feeds_the_partition_size_selection(oracle, torch_cuda):
    """centres -> centred search -> centred refinement -> fhevc_pu_shape_select_device on one stream with no host synchronisation, against the composed
    restatements"""
    import pu_shape_ref as sr
    torch = torch_cuda
    W, H, bd, qp, Rc, R = 176, 144, 8, 29, 14, 5
    pics = moving_pictures(W, H, bd, 2, seed=23)
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8))
    ctx = capi.Context(W, H, bd, max_frames=2)
    n = ctx.num_ctus
    st = torch.cuda.Stream()
    cen = Guarded(torch, n * 16)
    ints = {f: Guarded(torch, n * PER[f] * 16) for f in FAMS}
    qp_out = {f: Guarded(torch, n * PER[f] * 16) for f in FAMS}
    shapes = Guarded(torch, n * 85 * 16)
    torch.cuda.synchronize()
    s = st.cuda_stream
    ctx.motion_centres_device(d_luma.data_ptr(), 1, W, W * H, 2, cen.ptr, stream=s, qp=qp, coarse_range=Rc)
    ctx.motion_search_pu_centred_device(d_luma.data_ptr(), 1, W, W * H, 2, cen.ptr, ints["nodes"].ptr, ints["pu"].ptr, ints["small"].ptr, stream=s, qp=qp, search_range=R)
    ctx.motion_refine_pu_centred_device(d_luma.data_ptr(), 1, W, W * H, 2, cen.ptr, ints["nodes"].ptr, qp_out["nodes"].ptr, ints["pu"].ptr, qp_out["pu"].ptr,
                                        ints["small"].ptr, qp_out["small"].ptr, stream=s, qp=qp, max_range=R)
    ctx.pu_shape_select_device(qp_out["nodes"].ptr, qp_out["pu"].ptr, qp_out["small"].ptr, 1, shapes.ptr, stream=s)
    torch.cuda.synchronize()
    centres = expected(pics, bd, qp, Rc)
    same(cen.result((1, n)), centres, "centres")
    exp_i = expected_search(oracle, pics, bd, qp, R, centres)
    same_fams({f: ints[f].result((1, n, PER[f])) for f in FAMS}, exp_i, "search")
    exp_q = cr.centred_refine(oracle, pics[1], pics[0], bd, qp, R, centres[0], {f: exp_i[f][0] for f in FAMS})
    got_q = {f: qp_out[f].result((1, n, PER[f])).view(QDT)[0] for f in FAMS}
    same_q(got_q, exp_q, "refinement")
    rec, _ = sr.select(exp_q["nodes"][None], exp_q["pu"][None], exp_q["small"][None], W, H)
    h = shapes.t.cpu().numpy()[Guarded.GUARD:Guarded.GUARD + shapes.n].copy().view(sr.SDT).reshape(1, n, 85)
    sr.same(h, rec, "shapes")
    ctx.close()


# ---- 6. the reference's own results (tests/golden/ref_motion_centred.npz) ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(9))
def test_centred_search_and_refinement_vs_the_reference_golden(torch_cuda, k):
    """the reference's xPatternSearch / xPatternSearchFracDIF on the displaced reference picture: every entry whose reads stay inside the picture, in every
    field, counted per family; host forms on Pel planes at 10 / 12 bit, device forms on uint8 planes at 8 bit"""
    torch = torch_cuda
    c = cr.golden_cases()[k]
    ctx = capi.Context(c.W, c.H, c.bd, max_frames=2)
    ins = c.full_inputs()
    if c.bd == 8:
        d_luma = to_dev(torch, np.stack([c.ref, c.cur]).astype(np.uint8))
        got = {f: v[0] for f, v in search_dev(torch, ctx, d_luma, 0, c.W, c.W * c.H, 2, 1, c.qp, c.R, c.centres[None]).items()}
        fine = {f: v[0] for f, v in refine_dev(torch, ctx, d_luma, 0, c.W, c.W * c.H, 2, 1, c.qp, c.R, c.centres[None], {f: ins[f][None] for f in FAMS}).items()}
    else:
        (rb, org, stride), (cb, _, _) = pel(c.ref), pel(c.cur)
        got = dict(zip(FAMS, ctx.motion_search_pu_centred(cb, rb, c.centres, org, stride, qp=c.qp, search_range=c.R)))
        fine = dict(zip(FAMS, ctx.motion_refine_pu_centred(cb, rb, c.centres, org, stride, qp=c.qp, max_range=c.R, nodes=ins["nodes"], pus=ins["pu"], pus_small=ins["small"])))
    for f in FAMS:
        assert cr.same_flagged(got[f][c.ctus], c.search[f], c.inside[f], DT.names, (c, f)) == c.counts[f] > 0
        assert cr.same_flagged(fine[f][c.ctus], c.frac[f], c.inside_frac[f], QDT.names, (c, f)) == c.counts_frac[f] > 0
    ctx.close()


# ---- 7. the refinement's layouts, its grid, whole chains on two streams --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sample_bytes,bd", [(2, 10), (1, 8)])
def test_centred_refinement_layouts(oracle, torch_cuda, sample_bytes, bd):
    """planes between poison, odd origin and stride (uint8 and int16: the per-sample staging), odd centres, one centre out of range, a band, centres off a
    16-byte boundary; outputs between canaries"""
    torch = torch_cuda
    W, H, NF, qp, R = 104, 152, 3, 36, 8
    pics = moving_pictures(W, H, bd, NF, seed=60 + bd)
    stride, top, left = W + 13, 3, 7
    fs = stride * (H + 5) + 1
    dt = np.int16 if sample_bytes == 2 else np.uint8
    flat = np.full(NF * fs + 64, np.iinfo(dt).max, dt)
    org = top * stride + left
    for f, p in enumerate(pics):
        flat[f * fs + org:f * fs + org + H * stride].reshape(H, stride)[:, :W] = p
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    rng = np.random.default_rng(bd)
    vec = [[tuple(int(v) for v in rng.integers(-56, 57, size=2)) for _ in range(6)] for _ in range(NF - 1)]
    vec[0][3], vec[1][0] = (-57, 3), (11, 57)          # out of range: the CTU's markers, then the workgroup goes on with its next CTU
    centres = np.stack([cr.make_centres(v) for v in vec])
    ints = with_random_vectors(search_dev(torch, ctx, d_luma, org, stride, fs, NF, sample_bytes, qp, R, centres), centres, R, seed=bd)
    exp = [cr.centred_refine(oracle, pics[p + 1], pics[p], bd, qp, R, centres[p], {f: ints[f][p] for f in FAMS}) for p in range(NF - 1)]
    exp = {f: np.stack([e[f] for e in exp]) for f in FAMS}
    same_q(refine_dev(torch, ctx, d_luma, org, stride, fs, NF, sample_bytes, qp, R, centres, ints, centre_skew=4), exp, "whole")
    assert all((exp[f][0, 3]["cost_best"] == MARKER).all() and (exp[f][1, 0]["cost_best"] == MARKER).all() for f in FAMS)
    for rows in ((0, 1), (1, 3)):
        sl = slice(rows[0] * 2, rows[1] * 2)
        band = refine_dev(torch, ctx, d_luma, org, stride, fs, NF, sample_bytes, qp, R, np.ascontiguousarray(centres[:, sl]),
                          {f: np.ascontiguousarray(ints[f][:, sl]) for f in FAMS}, rows=rows, centre_skew=12)
        same_q(band, {f: exp[f][:, sl] for f in FAMS}, rows)
    ctx.close()


def test_centred_refinement_more_ctus_than_the_grid(oracle, torch_cuda):
    """9 pairs of 1024 x 576 are 1 296 CTUs: more than the four workgroups per CU of the square refinement's grid and the two of the PU refinement's; every
    third CTU has an out-of-range centre (markers, and the workgroup's next CTU is staged afresh), every 41st valid one is held to the restatement, and the
    CTUs with a zero centre to the wide refinement"""
    torch = torch_cuda
    W, H, NF, qp, R = 1024, 576, 10, 31, 3
    rng = np.random.default_rng(3)
    big = cr.texture(W + 4 * NF, H + 4 * NF, 8, 12, margin=0)
    pics = [np.clip(big[4 * f:4 * f + H, 4 * (NF - f):4 * (NF - f) + W] + rng.integers(-2, 3, size=(H, W)), 0, 255) for f in range(NF)]
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    assert (NF - 1) * n > 4 * 256
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8))
    centres = np.stack([cr.make_centres([((-4, 4), (0, 0), (60, -4))[(c + p) % 3] for c in range(n)]) for p in range(NF - 1)])
    usable = np.stack([cr.make_centres([((-4, 4), (0, 0), (0, 0))[(c + p) % 3] for c in range(n)]) for p in range(NF - 1)])
    ints = with_random_vectors(search_dev(torch, ctx, d_luma, 0, W, W * H, NF, 1, qp, R, usable), usable, R, seed=1)
    got = refine_dev(torch, ctx, d_luma, 0, W, W * H, NF, 1, qp, R, centres, ints)
    out_of_range = centres["mvx"] == 60
    for f in FAMS:
        assert (got[f][out_of_range]["cost_best"] == MARKER).all() and (got[f][out_of_range]["mvx"] == 0).all()
    for p in (0, NF - 2):
        ctus = [c for c in range(n) if (c + 7 * p) % 41 == 0]
        exp = cr.centred_refine(oracle, pics[p + 1], pics[p], 8, qp, R, centres[p], {f: ints[f][p] for f in FAMS}, ctus=ctus, planes=cr.rs.mr.Planes(pics[p], 8, 16))
        same_q({f: got[f][p][ctus] for f in FAMS}, {f: exp[f][ctus] for f in FAMS}, p)
    d_in = {f: to_dev(torch, ints[f]) for f in FAMS}
    g = {f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}
    ctx.motion_refine_pu_wide_device(d_luma.data_ptr(), 1, W, W * H, NF, d_in["nodes"].data_ptr(), g["nodes"].ptr, d_in["pu"].data_ptr(), g["pu"].ptr,
                                     d_in["small"].data_ptr(), g["small"].ptr, qp=qp, max_range=R)
    torch.cuda.synchronize()
    zero = centres["mvx"] == 0
    for f in FAMS:
        assert g[f].result((NF - 1, n, PER[f])).view(QDT)[zero].tobytes() == got[f][zero].tobytes(), f
    ctx.close()


def test_two_whole_chains_on_two_streams(oracle, torch_cuda):
    """centres -> search -> refinement -> partition-size selection, twice, with different QPs, ranges and (therefore) centres, in flight together on two streams
    with no host synchronisation"""
    import pu_shape_ref as sr
    torch = torch_cuda
    W, H, bd, NF = 176, 144, 8, 3
    pics = moving_pictures(W, H, bd, NF, seed=15)
    d_luma = to_dev(torch, np.stack(pics).astype(np.uint8))
    ctx = capi.Context(W, H, bd, max_frames=NF)
    n = ctx.num_ctus
    cases = [(24, 14, 8), (40, 2, 3)]      # QP, coarse range, search and refinement range
    streams = [torch.cuda.Stream() for _ in cases]
    bufs = [dict(cen=Guarded(torch, (NF - 1) * n * 16), ints={f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS},
                 fine={f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}, shapes=Guarded(torch, (NF - 1) * n * 85 * 16)) for _ in cases]
    torch.cuda.synchronize()
    p = d_luma.data_ptr()
    steps = (lambda q, Rc, R, s, b: ctx.motion_centres_device(p, 1, W, W * H, NF, b["cen"].ptr, stream=s, qp=q, coarse_range=Rc),
             lambda q, Rc, R, s, b: ctx.motion_search_pu_centred_device(p, 1, W, W * H, NF, b["cen"].ptr, b["ints"]["nodes"].ptr, b["ints"]["pu"].ptr, b["ints"]["small"].ptr,
                                                                        stream=s, qp=q, search_range=R),
             lambda q, Rc, R, s, b: ctx.motion_refine_pu_centred_device(p, 1, W, W * H, NF, b["cen"].ptr, b["ints"]["nodes"].ptr, b["fine"]["nodes"].ptr, b["ints"]["pu"].ptr,
                                                                        b["fine"]["pu"].ptr, b["ints"]["small"].ptr, b["fine"]["small"].ptr, stream=s, qp=q, max_range=R),
             lambda q, Rc, R, s, b: ctx.pu_shape_select_device(b["fine"]["nodes"].ptr, b["fine"]["pu"].ptr, b["fine"]["small"].ptr, NF - 1, b["shapes"].ptr, stream=s))
    for step in steps:          # interleaved: each stage of both chains before the next stage of either
        for (q, Rc, R), st, b in zip(cases, streams, bufs):
            step(q, Rc, R, st.cuda_stream, b)
    torch.cuda.synchronize()
    seen = []
    for (q, Rc, R), b in zip(cases, bufs):
        centres = expected(pics, bd, q, Rc)
        same(b["cen"].result((NF - 1, n)), centres, (q, "centres"))
        exp_i = expected_search(oracle, pics, bd, q, R, centres)
        same_fams({f: b["ints"][f].result((NF - 1, n, PER[f])) for f in FAMS}, exp_i, (q, "search"))
        exp_q = [cr.centred_refine(oracle, pics[k + 1], pics[k], bd, q, R, centres[k], {f: exp_i[f][k] for f in FAMS}) for k in range(NF - 1)]
        exp_q = {f: np.stack([e[f] for e in exp_q]) for f in FAMS}
        same_q({f: b["fine"][f].result((NF - 1, n, PER[f])).view(QDT) for f in FAMS}, exp_q, (q, "refinement"))
        rec, _ = sr.select(exp_q["nodes"], exp_q["pu"], exp_q["small"], W, H)
        h = b["shapes"].t.cpu().numpy()[Guarded.GUARD:Guarded.GUARD + b["shapes"].n].copy().view(sr.SDT).reshape(NF - 1, n, 85)
        sr.same(h, rec, (q, "shapes"))
        seen.append(centres)
    assert (seen[0]["mvx"] != seen[1]["mvx"]).any()
    ctx.close()
