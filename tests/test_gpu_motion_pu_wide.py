"""Config 4 (P slices): the three integer searches at HM's own SearchRange, fhevc_motion_search_pu_wide (the MR = 64 layouts of k_motion_pu.hip and
k_motion_pu_small.hip), on the MI355X: against what the reference itself returned (tests/golden/ref_pattern_search_pu_wide.npz), against the numpy
restatements (motion_pu_ref, motion_pu_small_ref; pinned to that file by test_oracle_golden_motion_pu_wide.py) and against the existing entry
points where they overlap.  Bit for bit, every field, markers included."""
import numpy as np
import pytest

import motion_golden as mg
import motion_pu_ref as pr
import motion_pu_small_ref as ps
import motion_pu_wide_cases as wc
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, Guarded, clip_planes, pel, pel_batch, same, to_dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

DT = capi.MOTION_DTYPE
FAMS = ("nodes", "pu", "small")
PER = {"nodes": capi.NODES_PER_CTU, "pu": capi.PUS_PER_CTU, "small": capi.PUS_SMALL_PER_CTU}


def run_dev(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, qp, R, rows=None, stream=None, fams=FAMS, d_luma=None):
    """one call over a device batch -> {family: [nf - 1, band CTUs, entries]} for the families asked for; guards checked, and the outputs of the
    families NOT asked for stay untouched"""
    rows_ = rows or (0, ctx.ctus_y)
    n = (rows_[1] - rows_[0]) * ctx.ctus_x
    d_luma = to_dev(torch, flat) if d_luma is None else d_luma
    g = {f: Guarded(torch, max((nf - 1) * n * PER[f] * 16, 16)) for f in FAMS}
    torch.cuda.synchronize()
    ctx.motion_search_pu_wide_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, *(g[f].ptr if f in fams else None for f in FAMS),
                                     rows=rows, stream=stream, qp=qp, search_range=R)
    torch.cuda.synchronize()
    assert all(g[f].untouched() for f in FAMS if f not in fams)
    return {f: g[f].result((nf - 1, n, PER[f])) for f in fams}


def expected(oracle, cur, ref, bd, qp, R, ctus=None):
    """{family: [numCtus, entries]} of the restatements in SAD mode; only `ctus` are filled"""
    nodes, pus = pr.expected(oracle, cur, ref, bd, qp, R, True, ctus=ctus)
    return {"nodes": nodes, "pu": pus, "small": ps.expected(oracle, cur, ref, bd, qp, R, True, ctus=ctus)}


def same_fams(got, exp, ctus=None, what=""):
    for f in got:
        a, b = (got[f], exp[f]) if ctus is None else (got[f][ctus], exp[f][ctus])
        same(a, b, (what, f))


def square_search(torch, ctx, d_luma_ptr, sample_bytes, stride, fs, nf, qp, R, n):
    """fhevc_motion_search_device in SAD mode -> [nf - 1, n, 85]"""
    ctx.set_motion_distortion("sad")
    out = Guarded(torch, (nf - 1) * n * 85 * 16)
    torch.cuda.synchronize()
    ctx.motion_search_device(d_luma_ptr, sample_bytes, stride, fs, nf, out.ptr, qp=qp, search_range=R)
    torch.cuda.synchronize()
    return out.result((nf - 1, n, 85))


# ---- 1. the reference's own results ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    return wc.wide_cases()


@pytest.mark.parametrize("k", range(8))
def test_golden_host_form_all_families_and_each_alone(cases, k):
    assert len(cases) == 8
    c = cases[k]
    (rb, org, stride), (cb, _, _) = pel(c.ref), pel(c.cur)
    ctx = capi.Context(c.W, c.H, c.bd)          # the distortion setting is left at its default (SATD): the entry point is SAD whatever it says
    got = dict(zip(FAMS, ctx.motion_search_pu_wide(cb, rb, org, stride, qp=c.qp, search_range=c.R)))
    for fam in FAMS:
        assert mg.same(got[fam][c.ctus], c.records(fam), (c, fam)) == wc.PER_CASE[fam]
        alone = ctx.motion_search_pu_wide(cb, rb, org, stride, qp=c.qp, search_range=c.R, nodes=fam == "nodes", pus=fam == "pu", pus_small=fam == "small")
        assert [o is None for o in alone] == [f != fam for f in FAMS]
        assert alone[FAMS.index(fam)].tobytes() == got[fam].tobytes(), (c, fam)
    ctx.close()


def test_golden_device_form_on_uint8_planes(cases, torch_cuda):
    torch = torch_cuda
    c8 = [c for c in cases if c.bd == 8]
    done = dict.fromkeys(FAMS, 0)
    for c in c8:
        ctx = capi.Context(c.W, c.H, 8, max_frames=2)
        flat = np.stack([c.ref, c.cur]).astype(np.uint8)
        got = run_dev(torch, ctx, flat, 0, c.W, c.W * c.H, 2, 1, c.qp, c.R)
        for fam in FAMS:
            done[fam] += mg.same(got[fam][0][c.ctus], c.records(fam), (c, fam))
        for fam in FAMS:   # each family alone: the others' outputs stay untouched (checked inside run_dev)
            assert run_dev(torch, ctx, flat, 0, c.W, c.W * c.H, 2, 1, c.qp, c.R, fams=(fam,))[fam].tobytes() == got[fam].tobytes(), (c, fam)
        ctx.close()
    assert len(c8) >= 5 and done == {f: len(c8) * n for f, n in wc.PER_CASE.items()}


# ---- 2. restatement on a ragged picture ----------------------------------------------------------------------------------------------------------------

# R = 9 and 10: the two remainders of (2 R + 1) mod 4 and a last block of dy that is moved up; 33 and 64: the ranges of the square golden.  The
# restatement costs about a second per CTU and family at R = 64: there it is held on CTUs 2 (48 wide) and 8 (48 x 16), at R = 33 on 0, 4 and 6
# too (whole, whole, 16 tall); the nodes of all nine CTUs against the square search in every case
@pytest.mark.parametrize("bd,qp,R,ctus", [(8, 30, 9, None), (8, 12, 10, None), (8, 41, 33, (0, 2, 4, 6, 8)), (8, 27, 64, (2, 8)), (10, 0, 9, None), (10, 51, 10, None),
                                          (10, 33, 64, (2, 8)), (12, 22, 9, None), (12, 37, 10, None), (12, 17, 33, (2, 4, 8)), (12, 32, 64, (6, 8))])
def test_ragged_picture_vs_restatement(oracle, torch_cuda, bd, qp, R, ctus):
    torch = torch_cuda
    W, H = 176, 144
    ys = frames.pan_clip(W, H, 2, seed=bd + qp + R, v_structure=R // 2 + 1, v_noise=-(R // 3) - 2)
    rp, cp = clip_planes(ys, bd, low_bits_seed=qp)
    flat, org, stride, fs = pel_batch([rp, cp])
    ctx = capi.Context(W, H, bd, max_frames=2)
    got = run_dev(torch, ctx, flat, org, stride, fs, 2, 2, qp, R)
    exp = expected(oracle, cp, rp, bd, qp, R, ctus=ctus)
    same_fams({f: v[0] for f, v in got.items()}, exp, ctus=list(ctus) if ctus else None, what=(bd, R))
    sq = square_search(torch, ctx, to_dev(torch, flat).data_ptr() + 2 * org, 2, stride, fs, 2, qp, R, ctx.num_ctus)
    assert sq.tobytes() == got["nodes"].tobytes()
    # markers exactly where the CU node's marker is, with a zero vector; valid entries of the whole picture counted
    nodes, pus, small = got["nodes"][0], got["pu"][0], got["small"][0]
    node_small = np.array([k for k, _, _ in ps.covered()])
    node_pu = np.array([k for k, _, _ in pr.covered()])
    for a, owner in ((pus, node_pu), (small, node_small)):
        mark = a["cost_best"] == pr.MARKER
        assert np.array_equal(mark, nodes["cost_best"][:, owner] == pr.MARKER)
        assert (a["satd_zero"][mark] == pr.MARKER).all() and (a["satd_best"][mark] == pr.MARKER).all() and (a["mvx"][mark] == 0).all() and (a["mvy"][mark] == 0).all()
    assert [int((a["cost_best"] != pr.MARKER).sum()) for a in (nodes, pus, small)] == [4 * 85 + 2 * 62 + 2 * 20 + 15, 4 * 124 + 2 * 72 + 2 * 16 + 12, 4 * 384 + 2 * 288 + 2 * 96 + 72]
    ctx.close()


@pytest.mark.parametrize("R,ctus", [(9, None), (64, (4, 8))])
def test_half_cut_16x16_nodes_small_pus(oracle, torch_cuda, R, ctus):
    """168 x 136: the last column of CTUs is 40 wide, the last row 8 tall -- 16x16 nodes cut in half, whose AMP entries are markers while the 8x8
    nodes inside the picture keep their 8x4 / 4x8 PUs"""
    torch = torch_cuda
    W, H, bd, qp = 168, 136, 8, 35
    ys = frames.pan_clip(W, H, 2, seed=R, v_structure=-7, v_noise=11)
    rp, cp = clip_planes(ys, bd)
    ctx = capi.Context(W, H, bd, max_frames=2)
    got = run_dev(torch, ctx, np.stack(ys), 0, W, W * H, 2, 1, qp, R)
    exp = expected(oracle, cp, rp, bd, qp, R, ctus=ctus)
    same_fams({f: v[0] for f, v in got.items()}, exp, ctus=list(ctus) if ctus else None, what=R)
    small = got["small"][0]
    c2 = small[2]["cost_best"] != pr.MARKER      # CTU 2: 40 wide -- 16x16 columns 0, 1 whole, column 2 cut in half; 8x8 columns 0..4
    assert int(c2[:128].sum()) == 4 * 2 * 8 and int(c2[128:].sum()) == 8 * 5 * 4
    ctx.close()


# ---- 3. long vectors are really found -------------------------------------------------------------------------------------------------------------------

def test_long_vectors_in_the_parts_of_a_cu(oracle, torch_cuda):
    """256 x 192, built by displacement of random samples.  CTU (1, 1): the top half moves by (+40, -3), the bottom half by (-37, +22); CTU (2, 1):
    the same two motions left / right.  CTU (1, 0): one 16x16 CU whose top quarter moves by (+51, +9) (2NxnU); CTU (2, 0): one 8x8 CU whose top half
    moves by (-44, +30) (8x4).  Both parts of the cutting shape return exactly those vectors with SAD 0 where the square node cannot"""
    W, H, bd, qp, R = 256, 192, 8, 30, 64
    rng = np.random.default_rng(7)
    ref = rng.integers(0, 256, size=(H, W)).astype(np.int64)
    big = np.pad(ref, 64, mode="edge")
    shifted = lambda dx, dy: big[64 + dy:64 + dy + H, 64 + dx:64 + dx + W]
    a, b, q, e = shifted(40, -3), shifted(-37, 22), shifted(51, 9), shifted(-44, 30)
    cur = ref.copy()
    cur[64:96, 64:128], cur[96:128, 64:128] = a[64:96, 64:128], b[96:128, 64:128]          # CTU 5 (1, 1): top / bottom
    cur[64:128, 128:160], cur[64:128, 160:192] = a[64:128, 128:160], b[64:128, 160:192]    # CTU 6 (2, 1): left / right
    cur[16:20, 80:96], cur[20:32, 80:96] = q[16:20, 80:96], a[20:32, 80:96]                # CTU 1 (1, 0): the 16x16 node at (16, 16), 2NxnU
    cur[8:12, 152:160], cur[12:16, 152:160] = e[8:12, 152:160], a[12:16, 152:160]          # CTU 2 (2, 0): the 8x8 node at (24, 8), 8x4
    (rb, org, stride), (cb, _, _) = pel(ref), pel(cur)
    ctx = capi.Context(W, H, bd)
    nodes, pus, small = ctx.motion_search_pu_wide(cb, rb, org, stride, qp=qp, search_range=R)
    vec = lambda r: (int(r["mvx"]), int(r["mvy"]))
    for ctu, shape in ((5, 0), (6, 1)):
        p0, p1 = pus[ctu, capi.motion_pu_index(0, shape, 0)], pus[ctu, capi.motion_pu_index(0, shape, 1)]
        assert vec(p0) == (40, -3) and vec(p1) == (-37, 22) and p0["satd_best"] == 0 and p1["satd_best"] == 0 and p0["satd_zero"] > 0
        assert nodes[ctu, 0]["satd_best"] > 0
    k16 = 5 + 1 * 4 + 1       # the 16x16 node at (16, 16)
    u0, u1 = small[1, capi.motion_pu_small_index(k16, 2, 0)], small[1, capi.motion_pu_small_index(k16, 2, 1)]
    assert vec(u0) == (51, 9) and vec(u1) == (40, -3) and u0["satd_best"] == 0 and u1["satd_best"] == 0 and nodes[1, k16]["satd_best"] > 0
    k8 = 21 + 1 * 8 + 3       # the 8x8 node at (24, 8)
    h0, h1 = small[2, capi.motion_pu_small_index(k8, 0, 0)], small[2, capi.motion_pu_small_index(k8, 0, 1)]
    assert vec(h0) == (-44, 30) and vec(h1) == (40, -3) and h0["satd_best"] == 0 and h1["satd_best"] == 0 and nodes[2, k8]["satd_best"] > 0
    # and the whole of those four CTUs is the restatement's
    same_fams({"nodes": nodes, "pu": pus, "small": small}, expected(oracle, cur, ref, bd, qp, R, ctus=(5, 2)), ctus=[5, 2])
    ctx.close()


# ---- 4. equalities with the existing entry points ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10, 12])
def test_small_ranges_equal_the_pu_entry_points(torch_cuda, bd):
    torch = torch_cuda
    W, H, NF, qp = 176, 144, 3, 28
    pics = clip_planes(frames.pan_clip(W, H, NF, seed=31 + bd, v_structure=3, v_noise=-2), bd, low_bits_seed=2)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    n = ctx.num_ctus
    for R in (1, 5, 8):
        ctx.set_motion_distortion("satd")
        got = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R, d_luma=d_luma)
        ctx.set_motion_distortion("sad")
        g = {f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}
        torch.cuda.synchronize()
        ctx.motion_search_pu_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, g["pu"].ptr, g["nodes"].ptr, qp=qp, search_range=R)
        ctx.motion_search_pu_small_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, g["small"].ptr, qp=qp, search_range=R)
        torch.cuda.synchronize()
        for f in FAMS:
            assert g[f].result(got[f].shape).tobytes() == got[f].tobytes(), (R, f)
    ctx.close()


@pytest.mark.parametrize("bd,R", [(8, 33), (8, 64), (10, 33), (10, 64)])
def test_nodes_equal_the_square_search_and_parts_sum_to_the_node(torch_cuda, bd, R):
    torch = torch_cuda
    W, H, NF, qp = 176, 144, 3, 19 + R // 3
    pics = clip_planes(frames.pan_clip(W, H, NF, seed=3 * bd + R, v_structure=17, v_noise=-23), bd, low_bits_seed=5)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    got = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R, d_luma=d_luma)
    assert square_search(torch, ctx, d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, qp, R, ctx.num_ctus).tobytes() == got["nodes"].tobytes()
    if bd == 8:   # SAD is additive and the shift is 0: the two parts of every valid shape sum to the node at the zero vector
        nz = got["nodes"]["satd_zero"].astype(np.int64)
        for fam, cov in (("pu", pr.covered()), ("small", ps.covered())):
            z = got[fam]["satd_zero"].astype(np.int64)
            owner = np.array([k for k, _, _ in cov])
            valid = got[fam]["cost_best"] != pr.MARKER
            pair = z[..., 0::2] + z[..., 1::2]
            assert valid.any() and np.array_equal(pair[valid[..., 0::2]], nz[..., owner[0::2]][valid[..., 0::2]]), fam


def test_generic_path_on_8_bit_planes_equals_the_default(torch_cuda, monkeypatch):
    """FHEVC_PU_WIDE=generic is read when a context is created: such a context sends 8-bit int16 planes down the generic path and writes the bytes
    the default context writes"""
    torch = torch_cuda
    W, H, qp = 176, 144, 31
    ys = frames.pan_clip(W, H, 2, seed=77, v_structure=21, v_noise=-30)
    flat, org, stride, fs = pel_batch([y.astype(np.int64) for y in ys])
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, 8, max_frames=2)
    monkeypatch.setenv("FHEVC_PU_WIDE", "generic")
    ctx_generic = capi.Context(W, H, 8, max_frames=2)
    monkeypatch.delenv("FHEVC_PU_WIDE")
    for R in (10, 33, 64):
        here = run_dev(torch, ctx, flat, org, stride, fs, 2, 2, qp, R, d_luma=d_luma)
        there = run_dev(torch, ctx_generic, flat, org, stride, fs, 2, 2, qp, R, d_luma=d_luma)
        for f in FAMS:
            assert there[f].tobytes() == here[f].tobytes(), (R, f)
    ctx.close()
    ctx_generic.close()


# ---- 5. layout ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,bd,shift", [(np.uint8, 8, 1), (np.uint8, 8, 0), (np.int16, 8, 1), (np.int16, 8, 0), (np.int16, 10, 1), (np.int16, 12, 0)])
def test_guarded_planes_poisoned_margins(oracle, torch_cuda, dtype, bd, shift):
    """nothing outside the picture is read for its value: margins, stride padding and the gap between frames hold poison.  shift 1: odd origin and
    odd stride, no row is aligned; shift 0: HM's alignment (the 16-byte / 8-byte staging loads)"""
    torch = torch_cuda
    W, H, NF, qp, R = 176, 144, 3, 27, 33
    ys = frames.pan_clip(W, H, NF, seed=9, v_structure=-14, v_noise=26)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3 * shift, shift=shift, frame_gap=5 * shift, poison=77)
    assert (stride % 2 == 1 and origin % 2 == 1) if shift else (stride % 8 == 0 and origin % 8 == 0)
    ctx = capi.Context(W, H, bd, max_frames=NF)
    got = run_dev(torch, ctx, flat, origin, stride, fstride, NF, np.dtype(dtype).itemsize, qp, R)
    for f in (0, 1):
        same_fams({k: v[f] for k, v in got.items()}, expected(oracle, pics[f + 1], pics[f], bd, qp, R, ctus=(2 + 6 * f,)), ctus=[2 + 6 * f], what=f)
    # the rest of the batch against the plain layout of the same pictures
    flat0, org0, stride0, fs0 = pel_batch(pics)
    plain = run_dev(torch, ctx, flat0, org0, stride0, fs0, NF, 2, qp, R)
    for k in FAMS:
        assert plain[k].tobytes() == got[k].tobytes(), k
    ctx.close()


def test_bands_between_canaries_an_empty_band_and_slot_11(torch_cuda):
    torch = torch_cuda
    W, H, NF, qp, R = 176, 144, 3, 33, 20
    pics = clip_planes(frames.pan_clip(W, H, NF, seed=12, v_structure=9, v_noise=-12), 10, low_bits_seed=4)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, 10, max_frames=NF)
    whole = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R, d_luma=d_luma)
    cw = ctx.ctus_x
    for rows in ((1, 2), (0, 1), (1, 3)):     # a band writes exactly its extent (guards checked inside run_dev)
        band = run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R, rows=rows, d_luma=d_luma)
        for f in FAMS:
            assert band[f].tobytes() == np.ascontiguousarray(whole[f][:, rows[0] * cw:rows[1] * cw]).tobytes(), (rows, f)
    # an empty band writes nothing, launches nothing and succeeds
    g = [Guarded(torch, 4096) for _ in FAMS]
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_search_pu_wide_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, g[0].ptr, g[1].ptr, g[2].ptr, rows=(2, 2), qp=qp, search_range=R)
    torch.cuda.synchronize()
    assert all(x.untouched() for x in g) and ctx.stats()["kernels_launched"] == launched
    # launches are counted, and timed under which = 11 and under no other slot
    ctx.enable_kernel_timing(True)
    for s in (4, 8, 9, 11):
        ctx.kernel_timing(s, reset=True)
    big = {f: Guarded(torch, (NF - 1) * cw * PER[f] * 16) for f in FAMS}
    ctx.motion_search_pu_wide_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, big["nodes"].ptr, big["pu"].ptr, big["small"].ptr, rows=(0, 1), qp=qp, search_range=R)
    torch.cuda.synchronize()
    ms, count = ctx.kernel_timing(11)
    assert count >= 1 and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + count and all(ctx.kernel_timing(s)[1] == 0 for s in (4, 8, 9))
    ctx.enable_kernel_timing(False)
    ctx.close()


def test_more_ctus_than_the_persistent_grid(oracle, torch_cuda):
    """22 pictures of 416 x 240 that alternate between two = 21 searches of 28 CTUs = 588 work items in one launch, more than two workgroups on each of
    256 CUs.  Every odd search equals the first, every even one the second; the first pair's CTUs 0, 13 and 27 (the last CTU of the launch is
    search 21's CTU 27) are held to the restatement"""
    torch = torch_cuda
    W, H, NF, qp, R = 416, 240, 22, 32, 33
    ys = frames.pan_clip(W, H, 2, seed=40, v_structure=12, v_noise=-19)
    pics = [ys[f % 2].astype(np.int64) for f in range(NF)]
    ctx = capi.Context(W, H, 8, max_frames=NF)
    assert (NF - 1) * ctx.num_ctus > 2 * 256
    got = run_dev(torch, ctx, np.stack([ys[f % 2] for f in range(NF)]), 0, W, W * H, NF, 1, qp, R)
    for fam in FAMS:
        for s in range(2, NF - 1):
            assert got[fam][s].tobytes() == got[fam][s % 2].tobytes(), (fam, s)
        assert got[fam][0].tobytes() != got[fam][1].tobytes()
    same_fams({k: v[0] for k, v in got.items()}, expected(oracle, pics[1], pics[0], 8, qp, R, ctus=(0, 13, 27)), ctus=[0, 13, 27])
    ctx.close()


# ---- 6. streams and the host form ------------------------------------------------------------------------------------------------------------------------

def test_two_streams_in_flight_with_different_qps_and_ranges(torch_cuda):
    """calls on two non-blocking streams, no synchronisation between them, different QPs and ranges: each output equals that of its own synchronous
    call (the bit costs travel with the launch; nothing is shared in HBM, nothing is kept in the context)"""
    torch = torch_cuda
    W, H, NF = 416, 240, 3
    pics = [y.astype(np.int64) for y in frames.pan_clip(W, H, NF, seed=21, v_structure=12, v_noise=-25)]
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    calls = [(12, 64), (47, 20), (30, 64), (22, 9)]
    alone = [run_dev(torch, ctx, flat, org, stride, fs, NF, 2, qp, R, d_luma=d_luma) for qp, R in calls]
    assert not np.array_equal(alone[0]["pu"]["cost_best"], alone[2]["pu"]["cost_best"])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [{f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS} for _ in calls]
    torch.cuda.synchronize()
    for i, (qp, R) in enumerate(calls):
        ctx.motion_search_pu_wide_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, outs[i]["nodes"].ptr, outs[i]["pu"].ptr, outs[i]["small"].ptr,
                                         stream=streams[i % 2].cuda_stream, qp=qp, search_range=R)
    torch.cuda.synchronize()
    for i in range(len(calls)):
        for f in FAMS:
            assert outs[i][f].result(alone[i][f].shape).tobytes() == alone[i][f].tobytes(), (i, f)
    ctx.close()


def test_host_form_equals_device_form(torch_cuda):
    torch = torch_cuda
    W, H, qp = 176, 144, 29
    for bd, R in ((8, 64), (10, 33), (12, 12)):
        pics = clip_planes(frames.pan_clip(W, H, 2, seed=60 + bd, v_structure=10, v_noise=-9), bd, low_bits_seed=1)
        (rb, org, stride), (cb, _, _) = pel(pics[0]), pel(pics[1])
        ctx = capi.Context(W, H, bd)
        host = dict(zip(FAMS, ctx.motion_search_pu_wide(cb, rb, org, stride, qp=qp, search_range=R)))
        dev = run_dev(torch, ctx, np.stack([rb, cb]), org, stride, rb.size, 2, 2, qp, R)
        for f in FAMS:
            assert host[f].tobytes() == dev[f][0].tobytes(), (bd, f)
            assert (host[f]["cost_best"] != pr.MARKER).any() and (host[f]["cost_best"] == pr.MARKER).any()
        ctx.close()


# ---- 7. rejected calls -------------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H = 416, 240
    ctx = capi.Context(W, H, 8)
    ctx10 = capi.Context(W, H, 10)
    n = ctx.num_ctus
    d_luma = torch.zeros((2 * W * H,), dtype=torch.int16, device="cuda")
    g = {f: Guarded(torch, n * PER[f] * 16) for f in FAMS}
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr(), sb=2, stride=W, fs=W * H, nf=2, rb=0, re=ctx.ctus_y, qp=32, sr=64, nodes=g["nodes"].ptr, pus=g["pu"].ptr,
                small=g["small"].ptr)
    bad = [dict(luma=None), dict(nodes=None, pus=None, small=None), dict(nf=1), dict(nf=0), dict(qp=-1), dict(qp=52), dict(sr=0), dict(sr=65), dict(sr=-8),
           dict(stride=W - 1), dict(rb=-1), dict(re=ctx.ctus_y + 1), dict(rb=3, re=2), dict(sb=3), dict(sb=0), dict(ctx=ctx10.h, sb=1)]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_search_pu_wide_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["sr"], a["nodes"],
                                                      a["pus"], a["small"], None)
    for change in bad:
        a = dict(good, **change)
        assert call(a) == capi.E_INVALID, change
        assert len(lib.fhevc_last_error(a["ctx"])) > 0, change          # the context says why
    assert call(dict(good, ctx=None)) == capi.E_INVALID
    torch.cuda.synchronize()
    assert all(x.untouched() for x in g.values()) and ctx.stats()["kernels_launched"] == launched and ctx10.stats()["kernels_launched"] == 0
    # the host form refuses the same way
    z = np.zeros((H, W), np.int16)
    res = np.zeros((n, 85), DT)
    for qp, sr, stride in ((52, 64, W), (-1, 64, W), (32, 0, W), (32, 65, W), (32, 64, W - 1)):
        assert lib.fhevc_motion_search_pu_wide(ctx.h, z.ctypes.data, z.ctypes.data, stride, qp, sr, res.ctypes.data, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_search_pu_wide(ctx.h, z.ctypes.data, z.ctypes.data, W, 32, 64, None, None, None) == capi.E_INVALID
    assert not res.view(np.uint8).any() and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted and writes the whole extent of all three outputs
    assert call(good) == capi.OK
    torch.cuda.synchronize()
    for f in FAMS:
        assert not (g[f].result((n, PER[f])).view(np.uint8).reshape(-1, 16) == CANARY).all(axis=1).any(), f
    ctx.close()
    ctx10.close()
