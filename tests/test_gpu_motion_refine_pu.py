"""Config 4 (P slices): the quarter-sample refinement of the PUs' vectors (k_motion_refine_pu.hip: all 508 PUs of a CTU, the 124 whose sides are
multiples of 8 and the 384 with a 4-sample side) on the MI355X against its numpy restatement (tests/motion_refine_pu_ref.py, pinned by
tests/test_motion_refine_pu_ref.py), bit for bit and field by field: SATD at the integer vector, the final quarter-sample vector, its SATD and
its cost."""
import numpy as np
import pytest

import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, Guarded, clip_planes, pel, pel_batch, to_dev, torch_cuda  # noqa: F401
from test_motion_refine_ref import textured

pytestmark = pytest.mark.gpu

QDT = capi.MOTION_QPEL_DTYPE
PER = {"pu": capi.PUS_PER_CTU, "small": capi.PUS_SMALL_PER_CTU}
FAMS = ("pu", "small")
NODE_OF = {"pu": np.array([k for k, _, _ in mp.covered()]), "small": np.array([k for k, _, _ in ps.covered()])}


def same(got, exp, what=""):
    for k in QDT.names:
        assert np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:5], got[k][got[k] != exp[k]][:5], exp[k][got[k] != exp[k]][:5])


def band_ctus(ctx, rows):
    rows = rows or (0, ctx.ctus_y)
    return (rows[1] - rows[0]) * ctx.ctus_x


def search_dev(torch, ctx, d_luma_ptr, sb, stride, fs, nf, qp, R, rows=None):
    """both PU searches over a device batch -> {"pu": [nf - 1, band CTUs, 124], "small": [.., 384]} MOTION_DTYPE"""
    n = band_ctus(ctx, rows)
    g = {fam: Guarded(torch, (nf - 1) * n * PER[fam] * 16) for fam in FAMS}
    torch.cuda.synchronize()
    ctx.motion_search_pu_device(d_luma_ptr, sb, stride, fs, nf, g["pu"].ptr, rows=rows, qp=qp, search_range=R)
    ctx.motion_search_pu_small_device(d_luma_ptr, sb, stride, fs, nf, g["small"].ptr, rows=rows, qp=qp, search_range=R)
    torch.cuda.synchronize()
    return {fam: g[fam].result((nf - 1, n, PER[fam])) for fam in FAMS}


def refine_dev(torch, ctx, d_luma_ptr, sb, stride, fs, nf, qp, R, ins, rows=None, stream=None):
    """one launch of the refinement over a device batch; ins: {family: [nf - 1, band CTUs, per CTU]} (a family left out: its pair is NULL)
    -> {family: the same shape of MOTION_QPEL_DTYPE}; guards checked"""
    n = band_ctus(ctx, rows)
    d_in = {fam: to_dev(torch, a) for fam, a in ins.items()}
    g = {fam: Guarded(torch, max((nf - 1) * n * PER[fam] * 16, 16)) for fam in ins}
    pair = [p for fam in FAMS for p in ((d_in[fam].data_ptr(), g[fam].ptr) if fam in ins else (None, None))]
    torch.cuda.synchronize()
    ctx.motion_refine_pu_device(d_luma_ptr, sb, stride, fs, nf, *pair, rows=rows, stream=stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    return {fam: g[fam].result((nf - 1, n, PER[fam])).view(QDT) for fam in ins}


def expected_batch(oracle, pics, bd, qp, R, ins, ctus=None):
    """{family: [nf - 1, numCtus, per CTU]} of the restatement for whole pictures"""
    return {fam: np.stack([rp.expected(oracle, pics[f], pics[f - 1], bd, qp, a[f - 1], R, fam, ctus=ctus) for f in range(1, len(pics))]) for fam, a in ins.items()}


def random_entries(shape, seed, lo=-12, hi=12):
    """input entries of random bytes with vectors from lo .. hi: nothing but mvx / mvy may matter"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=shape + (16,), dtype=np.uint8).view(capi.MOTION_DTYPE).reshape(shape)
    a["mvx"], a["mvy"] = rng.integers(lo, hi + 1, size=shape), rng.integers(lo, hi + 1, size=shape)
    return a


# ---- 1. ragged picture, host form, both families --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,qp,R,sad", [(8, 0, 1, False), (8, 51, 8, True), (10, 32, 8, False), (10, 0, 5, True), (12, 32, 1, False), (12, 51, 5, True)])
def test_ragged_picture_vs_restatement(oracle, bd, qp, R, sad):
    W, H = 168, 136   # 3 x 3 CTUs, the last column 40 wide, the last row 8 tall: a 16x16 node cut in half next to whole ones, 8x8 nodes alone
    ys = frames.pan_clip(W, H, 2, seed=5 + bd + qp + R, v_structure=2, v_noise=-3)
    rpic, cpic = clip_planes(ys, bd, low_bits_seed=qp)
    (rb, org, stride), (cb, _, _) = pel(rpic), pel(cpic)
    ctx = capi.Context(W, H, bd)
    ctx.set_motion_distortion("sad" if sad else "satd")     # the searches' distortion; the refinement is Hadamard whatever this says
    ins = {"pu": ctx.motion_search_pu(cb, rb, org, stride, qp=qp, search_range=R), "small": ctx.motion_search_pu_small(cb, rb, org, stride, qp=qp, search_range=R)}
    out = dict(zip(FAMS, ctx.motion_refine_pu(cb, rb, org, stride, qp=qp, max_range=R, pus=ins["pu"], pus_small=ins["small"])))
    valid_pu = mp.expected(oracle, cpic, rpic, bd, qp, 1, True)[1]["cost_best"] != mp.MARKER     # the geometry's markers, from the search's restatement
    for fam in FAMS:
        same(out[fam], rp.expected(oracle, cpic, rpic, bd, qp, ins[fam], R, fam), fam)
        # markers exactly where the search's markers sit, with zero vectors
        mark = out[fam]["cost_best"] == rp.MARKER
        assert np.array_equal(mark, ins[fam]["cost_best"] == rp.MARKER)
        assert (out[fam]["satd_int"][mark] == rp.MARKER).all() and (out[fam]["satd_best"][mark] == rp.MARKER).all()
        assert (out[fam]["mvx"][mark] == 0).all() and (out[fam]["mvy"][mark] == 0).all()
        assert (out[fam]["satd_int"][~mark] != rp.MARKER).all()
    mark = out["small"]["cost_best"] == rp.MARKER
    for c, amp, small in ((0, 128, 256), (2, 64, 160), (6, 0, 32), (8, 0, 20)):   # whole; 40 wide: eight 16x16, forty 8x8 nodes; 8 tall: eight 8x8; the corner: five
        assert int((~mark[c, :128]).sum()) == amp and int((~mark[c, 128:]).sum()) == small, c
        assert int((out["pu"]["cost_best"][c] != rp.MARKER).sum()) == int(valid_pu[c].sum()), c
    assert int(valid_pu[0].sum()) == 124 and int(valid_pu[2].sum()) == 2 * 12 + 8 * 4 and int(valid_pu[6].sum()) == 0   # 40 wide: two 32x32 nodes, eight 16x16 nodes
    ctx.close()


# ---- 2. two half-sample motions inside one CU ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fa,fb", [((2, 0), (0, 2)), ((2, 2), (2, 0))])
def test_two_half_sample_motions_inside_one_cu(oracle, fa, fb):
    """the picture tests/test_motion_refine_pu_ref.py builds with the filter itself: 256 x 64, one CTU each for 2NxnU and nLx2N of the 16x16 CUs and
    for the 8x4 and 4x8 halves of the 8x8 CUs, and a 64 x 64 one for 2NxN of the 32x32 CUs.  Fed the integer vectors, both parts end at exactly
    their quarter-unit vectors with no distortion left"""
    bd, qp, a, b = 10, 4, (2, -1), (-3, 2)
    qa, qb = (4 * a[0] + fa[0], 4 * a[1] + fa[1]), (4 * b[0] + fb[0], 4 * b[1] + fb[1])
    index = {"pu": capi.motion_pu_index, "small": capi.motion_pu_small_index}
    for kinds in (["2NxnU@16", "nLx2N@16", "2NxN@8", "Nx2N@8"], ["2NxN@32"]):
        W, H = 64 * len(kinds), 64
        ref = textured(W, H, bd, 51)
        planes = mr.Planes(ref, bd, 16)
        cur = rp.two_motion_picture(planes, kinds, qa, qb)
        (rb, org, stride), (cb, _, _) = pel(ref), pel(cur)
        ctx = capi.Context(W, H, bd)
        ins = {fam: rp.two_motion_inputs(kinds, fam, a, b) for fam in FAMS}
        out = dict(zip(FAMS, ctx.motion_refine_pu(cb, rb, org, stride, qp=qp, max_range=4, pus=ins["pu"], pus_small=ins["small"])))
        for fam in FAMS:
            same(out[fam], rp.expected(oracle, cur, ref, bd, qp, ins[fam], 4, fam, planes=planes), fam)
        for ctu, kind in enumerate(kinds):
            fam, shape, nodes, _ = rp.TWO_MOTION_KINDS[kind]
            for k in nodes:
                p0, p1 = out[fam][ctu, index[fam](k, shape, 0)], out[fam][ctu, index[fam](k, shape, 1)]
                assert (int(p0["mvx"]), int(p0["mvy"])) == qa and (int(p1["mvx"]), int(p1["mvy"])) == qb, (kind, k)
                assert p0["satd_best"] == 0 and p1["satd_best"] == 0 and p0["satd_int"] > 0 and p1["satd_int"] > 0, (kind, k)
        ctx.close()


# ---- 3. random input bytes; 4. uint8 planes --------------------------------------------------------------------------------------------------------

def test_random_input_bytes_one_family_at_a_time_and_both(oracle, torch_cuda):
    """only mvx / mvy of the input are read, and a vector beyond max_range gives the marker instead of a read outside the window; one family with
    the other pair NULL writes the bytes the call with both writes"""
    torch = torch_cuda
    W, H, NF, bd, qp, R = 168, 136, 2, 10, 26, 8
    pics = clip_planes(frames.pan_clip(W, H, NF, seed=31, v_structure=3, v_noise=4), bd, low_bits_seed=8)
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    ins = {fam: random_entries((NF - 1, ctx.num_ctus, PER[fam]), 70 + i) for i, fam in enumerate(FAMS)}
    d_luma = to_dev(torch, flat)
    both = refine_dev(torch, ctx, d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, qp, R, ins)
    exp = expected_batch(oracle, pics, bd, qp, R, ins)
    for fam in FAMS:
        same(both[fam], exp[fam], fam)
        too_long = (np.abs(ins[fam]["mvx"]) > R) | (np.abs(ins[fam]["mvy"]) > R)
        assert too_long.any() and (both[fam]["cost_best"][too_long] == rp.MARKER).all() and (both[fam]["cost_best"] != rp.MARKER).any()
        alone = refine_dev(torch, ctx, d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, qp, R, {fam: ins[fam]})
        assert alone[fam].tobytes() == both[fam].tobytes(), fam
    ctx.close()


def test_uint8_planes_equal_int16_planes(oracle, torch_cuda):
    torch = torch_cuda
    W, H, NF, qp, R = 168, 136, 3, 30, 6
    ys = frames.pan_clip(W, H, NF, seed=4, v_structure=4, v_noise=-2)
    pics = [y.astype(np.int64) for y in ys]
    ctx = capi.Context(W, H, 8, max_frames=NF)
    flat, org, stride, fs = pel_batch(pics)
    d16, d8 = to_dev(torch, flat), to_dev(torch, np.stack(ys))
    ins = search_dev(torch, ctx, d16.data_ptr() + 2 * org, 2, stride, fs, NF, qp, R)
    o16 = refine_dev(torch, ctx, d16.data_ptr() + 2 * org, 2, stride, fs, NF, qp, R, ins)
    o8 = refine_dev(torch, ctx, d8.data_ptr(), 1, W, W * H, NF, qp, R, ins)
    exp = expected_batch(oracle, pics, 8, qp, R, ins)
    for fam in FAMS:
        same(o16[fam], exp[fam], fam)
        assert o8[fam].tobytes() == o16[fam].tobytes(), fam
    ctx.close()


# ---- 5. guarded planes; 6. bands -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [1, 0], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("dtype,bd", [(np.int16, 10), (np.int16, 12), (np.uint8, 8)])
def test_guarded_planes_poisoned_margins_both_load_paths(oracle, torch_cuda, dtype, bd, shift):
    """nothing outside the picture is read for its value: margins, stride padding and the gap between frames hold poison.  shift 1: odd origin and
    odd stride, no row is aligned (the scalar staging path); shift 0: HM's alignment (the 8-byte / 4-byte staging path).  Outputs between 4 KiB
    canaries are written over exactly their extent (refine_dev)"""
    torch = torch_cuda
    W, H, NF, qp, R = 168, 136, 2, 27, 7
    ys = frames.pan_clip(W, H, NF, seed=9, v_structure=-4, v_noise=6)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3 * shift, shift=shift, frame_gap=5 * shift, poison=77)
    assert (stride % 2 == 1 and origin % 2 == 1) if shift else (stride % 8 == 0 and origin % 8 == 0)
    sb = np.dtype(dtype).itemsize
    ctx = capi.Context(W, H, bd, max_frames=NF)
    d_luma = to_dev(torch, flat)
    ins = {fam: random_entries((NF - 1, ctx.num_ctus, PER[fam]), 90 + bd + i, -R, R) for i, fam in enumerate(FAMS)}
    out = refine_dev(torch, ctx, d_luma.data_ptr() + sb * origin, sb, stride, fstride, NF, qp, R, ins)
    exp = expected_batch(oracle, pics, bd, qp, R, ins)
    for fam in FAMS:
        same(out[fam], exp[fam], fam)
    ctx.close()


def test_bands_between_canaries_and_an_empty_band(oracle, torch_cuda):
    torch = torch_cuda
    W, H, NF, bd, qp, R = 168, 136, 3, 10, 33, 4
    pics = clip_planes(frames.pan_clip(W, H, NF, seed=12), bd, low_bits_seed=4)
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    d_luma = to_dev(torch, flat)
    lp = d_luma.data_ptr() + 2 * org
    ins = search_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R)
    whole = refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R, ins)
    exp = expected_batch(oracle, pics, bd, qp, R, ins)
    for fam in FAMS:
        same(whole[fam], exp[fam], fam)
    cw = ctx.ctus_x
    for rows in ((1, 3), (0, 1)):     # compact over the band, written over exactly its extent (guards checked inside refine_dev)
        band_in = {fam: np.ascontiguousarray(ins[fam][:, rows[0] * cw:rows[1] * cw]) for fam in FAMS}
        got = refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R, band_in, rows=rows)
        for fam in FAMS:
            assert got[fam].tobytes() == np.ascontiguousarray(whole[fam][:, rows[0] * cw:rows[1] * cw]).tobytes(), (rows, fam)
    # an empty band writes nothing, launches nothing and succeeds
    d_in = {fam: to_dev(torch, ins[fam]) for fam in FAMS}
    outs = {fam: Guarded(torch, 4096) for fam in FAMS}
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_refine_pu_device(lp, 2, stride, fs, NF, d_in["pu"].data_ptr(), outs["pu"].ptr, d_in["small"].data_ptr(), outs["small"].ptr, rows=(2, 2), qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert outs["pu"].untouched() and outs["small"].untouched() and ctx.stats()["kernels_launched"] == launched
    # a launch is counted, and timed under which = 10
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(10, reset=True)
    big = Guarded(torch, (NF - 1) * cw * PER["small"] * 16)
    ctx.motion_refine_pu_device(lp, 2, stride, fs, NF, None, None, d_in["small"].data_ptr(), big.ptr, rows=(0, 1), qp=qp, max_range=R)
    torch.cuda.synchronize()
    ms, count = ctx.kernel_timing(10)
    assert count == 1 and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + 1 and ctx.kernel_timing(7)[1] == 0 and ctx.kernel_timing(9)[1] == 0
    ctx.enable_kernel_timing(False)
    ctx.close()


# ---- 7. more CTUs than the launch grid -------------------------------------------------------------------------------------------------------------

def test_1080p_grid_stride(oracle, torch_cuda):
    """three 1080p pictures = two pairs = 1020 CTUs in one launch.  The launch's grid is capped at TWO workgroups per CU (the kernel's residency:
    k_motion_refine_pu.hip, WG_PER_CU), 512 on the MI355X's 256 CUs, so every workgroup walks its grid-stride loop and work items 512 .. 1019 are
    second visits.  The restatement on a fixed sample of 34 CTUs; the marker pattern everywhere"""
    torch = torch_cuda
    W, H, NF, qp, R = 1920, 1080, 3, 32, 8
    ys = frames.pan_clip(W, H, NF)
    pics = [y.astype(np.int64) for y in ys]
    planes = [frames.to_pel_plane(y, 8) for y in ys]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    assert n == 510 and (NF - 1) * n > 2 * 256
    ins = {fam: random_entries((NF - 1, n, PER[fam]), 40 + i, -9, 9) for i, fam in enumerate(FAMS)}
    d_luma = to_dev(torch, flat)
    out = refine_dev(torch, ctx, d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, qp, R, ins)
    # pair 0: the first CTU, the right column, the 56-tall bottom row; pair 1 = work items 510 ..: 512 and beyond are past the grid cap; 509 = the last
    sample = {0: [0, 29, 59, 263, 480, 495, 509], 1: [0, 1, 2, 3, 17, 29, 30, 89, 119, 200, 255, 256, 257, 300, 333, 389, 401, 449, 479, 480, 481, 490, 499, 505, 507, 508, 509]}
    assert sum(len(v) for v in sample.values()) >= 32
    for f, ctus in sample.items():
        for fam in FAMS:
            exp = rp.expected(oracle, pics[f + 1], pics[f], 8, qp, ins[fam][f], R, fam, ctus=ctus)
            same(out[fam][f][ctus], exp[ctus], (f, fam))
    for fam in FAMS:
        k = NODE_OF[fam]
        size = np.where(k == 0, 64, np.where(k < 5, 32, np.where(k < 21, 16, 8)))
        y0 = np.array([mp.node_rect(int(v))[1] for v in k])
        inside = np.ones((n, PER[fam]), bool)
        inside[480:] = (y0 + size <= 56)[None, :]            # the last CTU row is 56 tall; 1920 = 30 whole CTUs
        valid = inside[None] & (np.abs(ins[fam]["mvx"]) <= R) & (np.abs(ins[fam]["mvy"]) <= R)
        assert np.array_equal(out[fam]["cost_best"] != rp.MARKER, valid), fam
        assert (out[fam]["mvx"][~valid] == 0).all() and (out[fam]["mvy"][~valid] == 0).all() and (out[fam]["satd_best"][~valid] == rp.MARKER).all()
    ctx.close()


# ---- 8. / 9. streams; 10. the host form; 11. rejected calls ----------------------------------------------------------------------------------------

def test_two_streams_in_flight_with_different_qps(torch_cuda):
    """calls on two non-blocking streams, no synchronisation between them, different QPs and ranges: each output equals that of its own synchronous
    call (the vector costs travel with the launch; nothing is shared in HBM)"""
    torch = torch_cuda
    W, H, NF = 416, 240, 3
    pics = [y.astype(np.int64) for y in frames.pan_clip(W, H, NF, seed=21, v_structure=2, v_noise=-5)]
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    d_luma = to_dev(torch, flat)
    lp = d_luma.data_ptr() + 2 * org
    ins = {fam: random_entries((NF - 1, n, PER[fam]), 55 + i, -8, 8) for i, fam in enumerate(FAMS)}
    calls = [(12, 8), (47, 3), (30, 8), (22, 5)]
    alone = [refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R, ins) for qp, R in calls]
    assert not np.array_equal(alone[0]["pu"]["cost_best"], alone[2]["pu"]["cost_best"])
    d_in = {fam: to_dev(torch, ins[fam]) for fam in FAMS}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [{fam: Guarded(torch, (NF - 1) * n * PER[fam] * 16) for fam in FAMS} for _ in calls]
    torch.cuda.synchronize()
    for i, (qp, R) in enumerate(calls):
        ctx.motion_refine_pu_device(lp, 2, stride, fs, NF, d_in["pu"].data_ptr(), outs[i]["pu"].ptr, d_in["small"].data_ptr(), outs[i]["small"].ptr,
                                    stream=streams[i % 2].cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    for i in range(len(calls)):
        for fam in FAMS:
            assert outs[i][fam].result(alone[i][fam].shape).tobytes() == alone[i][fam].tobytes(), (i, fam)
    ctx.close()


def test_search_and_refinement_on_one_stream_without_a_host_synchronisation(torch_cuda):
    torch = torch_cuda
    W, H, NF, bd, qp, R = 416, 240, 3, 10, 28, 6
    pics = clip_planes(frames.pan_clip(W, H, NF, seed=23, v_structure=2, v_noise=3), bd, low_bits_seed=2)
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    n = ctx.num_ctus
    d_luma = to_dev(torch, flat)
    lp = d_luma.data_ptr() + 2 * org
    ins = search_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R)            # the synchronised sequence
    exp = refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R, ins)
    st = torch.cuda.Stream()
    mid = {fam: Guarded(torch, (NF - 1) * n * PER[fam] * 16) for fam in FAMS}
    out = {fam: Guarded(torch, (NF - 1) * n * PER[fam] * 16) for fam in FAMS}
    torch.cuda.synchronize()
    ctx.motion_search_pu_device(lp, 2, stride, fs, NF, mid["pu"].ptr, stream=st.cuda_stream, qp=qp, search_range=R)
    ctx.motion_search_pu_small_device(lp, 2, stride, fs, NF, mid["small"].ptr, stream=st.cuda_stream, qp=qp, search_range=R)
    ctx.motion_refine_pu_device(lp, 2, stride, fs, NF, mid["pu"].ptr, out["pu"].ptr, mid["small"].ptr, out["small"].ptr, stream=st.cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    for fam in FAMS:
        assert mid[fam].result(ins[fam].shape).tobytes() == ins[fam].tobytes(), fam
        assert out[fam].result(exp[fam].shape).tobytes() == exp[fam].tobytes(), fam
        assert (exp[fam]["cost_best"] != rp.MARKER).any()
    ctx.close()


def test_host_form_equals_device_form(torch_cuda):
    torch = torch_cuda
    W, H, qp = 168, 136, 29
    for bd, R in ((8, 8), (10, 3), (12, 6)):
        pics = clip_planes(frames.pan_clip(W, H, 2, seed=60 + bd), bd, low_bits_seed=1)
        (rb, org, stride), (cb, _, _) = pel(pics[0]), pel(pics[1])
        ctx = capi.Context(W, H, bd)
        ins = {fam: random_entries((1, ctx.num_ctus, PER[fam]), bd + i, -R, R) for i, fam in enumerate(FAMS)}
        host = dict(zip(FAMS, ctx.motion_refine_pu(cb, rb, org, stride, qp=qp, max_range=R, pus=ins["pu"][0], pus_small=ins["small"][0])))
        d_luma = to_dev(torch, np.stack([rb, cb]))
        dev = refine_dev(torch, ctx, d_luma.data_ptr() + 2 * org, 2, stride, rb.size, 2, qp, R, ins)
        for fam in FAMS:
            assert host[fam].tobytes() == dev[fam][0].tobytes(), (bd, fam)
            assert (host[fam]["cost_best"] != rp.MARKER).any() and (host[fam]["cost_best"] == rp.MARKER).any()
        # one family alone: the other comes back as None
        only, none = ctx.motion_refine_pu(cb, rb, org, stride, qp=qp, max_range=R, pus=ins["pu"][0])
        assert none is None and only.tobytes() == host["pu"].tobytes()
        none, only = ctx.motion_refine_pu(cb, rb, org, stride, qp=qp, max_range=R, pus_small=ins["small"][0])
        assert none is None and only.tobytes() == host["small"].tobytes()
        ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H = 416, 240
    ctx = capi.Context(W, H, 8)
    ctx10 = capi.Context(W, H, 10)
    n = ctx.num_ctus
    d_luma = torch.zeros((2 * W * H,), dtype=torch.int16, device="cuda")
    d_in = {fam: torch.zeros((n * PER[fam] * 16,), dtype=torch.uint8, device="cuda") for fam in FAMS}
    out = {fam: Guarded(torch, n * PER[fam] * 16) for fam in FAMS}
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr(), sb=2, stride=W, fs=W * H, nf=2, rb=0, re=ctx.ctus_y, qp=32, mr=8, pus=d_in["pu"].data_ptr(), opus=out["pu"].ptr,
                small=d_in["small"].data_ptr(), osmall=out["small"].ptr)
    bad = [dict(luma=None), dict(pus=None, opus=None, small=None, osmall=None), dict(pus=None), dict(opus=None), dict(small=None), dict(osmall=None),
           dict(pus=None, opus=None, osmall=None), dict(nf=1), dict(nf=0), dict(qp=-1), dict(qp=52), dict(mr=0), dict(mr=9), dict(mr=64), dict(mr=-8),
           dict(stride=W - 1), dict(rb=-1), dict(re=ctx.ctus_y + 1), dict(rb=3, re=2), dict(sb=3), dict(sb=0), dict(ctx=ctx10.h, sb=1)]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_refine_pu_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["mr"], a["pus"], a["opus"],
                                                 a["small"], a["osmall"], None)
    for change in bad:
        a = dict(good, **change)
        assert call(a) == capi.E_INVALID, change
        assert len(lib.fhevc_last_error(a["ctx"])) > 0, change          # the context says why
    assert call(dict(good, ctx=None)) == capi.E_INVALID
    torch.cuda.synchronize()
    assert out["pu"].untouched() and out["small"].untouched() and ctx.stats()["kernels_launched"] == launched and ctx10.stats()["kernels_launched"] == 0
    # the host form refuses the same way
    z = np.zeros((H, W), np.int16)
    hin = {fam: np.zeros((n, PER[fam]), capi.MOTION_DTYPE) for fam in FAMS}
    res = {fam: np.zeros((n, PER[fam]), QDT) for fam in FAMS}
    p = lambda a: a.ctypes.data
    for qp, mrange, stride in ((52, 8, W), (-1, 8, W), (32, 0, W), (32, 9, W), (32, 8, W - 1)):
        assert lib.fhevc_motion_refine_pu(ctx.h, p(z), p(z), stride, qp, mrange, p(hin["pu"]), p(res["pu"]), p(hin["small"]), p(res["small"])) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu(ctx.h, p(z), p(z), W, 32, 8, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu(ctx.h, p(z), p(z), W, 32, 8, p(hin["pu"]), None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu(ctx.h, p(z), p(z), W, 32, 8, None, None, None, p(res["small"])) == capi.E_INVALID
    assert not res["pu"].view(np.uint8).any() and not res["small"].view(np.uint8).any() and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted and writes the whole extent of both outputs
    assert call(good) == capi.OK
    torch.cuda.synchronize()
    for fam in FAMS:
        assert not (out[fam].result((n, PER[fam])).view(np.uint8).reshape(-1, 16) == CANARY).all(axis=1).any()
    ctx.close()
    ctx10.close()
