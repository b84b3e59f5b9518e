"""Config 4 (P slices): the merge stage (k_motion_merge.hip), the tree decision that takes its costs (the merge instantiation of k_p_tree.hip) and
fhevc_p_tree_merge_frame on the MI355X, bit for bit and field by field against the Python restatement tests/motion_merge_ref.py (pinned without a GPU by
tests/test_motion_merge_ref.py).  Nothing is compared with a kernel's own output except where two launches must give the same bytes.

Pictures are 200 x 136 = 4 x 3 CTUs, ragged by 8 samples on both sides, so L, A, AR and AL cross CTU borders and the last column and row hold nodes that
are not INSIDE; the constructed cases bring their own sizes (tests/motion_merge_cases.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import motion_merge_cases as mc
import motion_merge_ref as mg
import motion_refine_ref as mr
import p_tree_cases as tc
import p_tree_ref as tr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, clip_planes, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

W, H = 200, 136
CW, CH = 4, 3
N = CW * CH
MDT, QDT, SDT, TDT, IDT = capi.MOTION_MERGE_DTYPE, capi.MOTION_QPEL_DTYPE, capi.SHAPE_DTYPE, capi.TREE_DTYPE, capi.MOTION_DTYPE
ALL = (True, True, True)
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


def run_merge(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, refined, qp, max_range, rows=None, stream=None):
    """refined [nf - 1, band CTUs, 85] -> the merge records of the same shape; the output lies between canaries"""
    d_luma, d_ref = to_dev(torch, flat), to_dev(torch, refined)
    out = Guarded(torch, refined.size * 16)
    torch.cuda.synchronize()
    ctx.motion_merge_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, d_ref.data_ptr(), out.ptr, rows=rows, stream=stream,
                            qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    return out.result(MDT, refined.shape)


def expected_batch(oracle, pics, bd, qp, refined, max_range, rows=None, w=W, h=H):
    """pics: [H, W] samples per frame; refined [nf - 1, band CTUs, 85] compact over the band"""
    out = np.zeros(refined.shape, MDT)
    for f in range(1, len(pics)):
        buf, org, stride = pel(pics[f])
        out[f - 1] = mg.expected(oracle, buf.reshape(-1), org, stride, pics[f - 1], w, h, bd, qp, refined[f - 1], max_range, rows=rows)
    return out


def check_markers(got):
    """nodes that are not INSIDE carry the marker record, all others a list"""
    for c in range(N):
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            ins = mg.inside(W, H, lvl, (c % CW) * (1 << lvl) + bx, (c // CW) * (1 << lvl) + by)
            for r in got[:, c, k]:
                assert (tuple(r) == mg.INVALID) == (not ins) and (1 <= r["num"] <= 5) == ins and r["pad"] == 0, (c, k, r)


def noise_pictures(seed, nf, bd=8):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, size=(H, W)).astype(np.int64) for _ in range(nf)]


def random_refined(rng, shape, max_range):
    """refined records of random bytes; vectors drawn from four near ones (so that every pruning pair fires), one record in ten out of reach (one
    quarter sample beyond it, or anywhere), one in seven marked"""
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), QDT).reshape(shape).copy()
    reach = 4 * max_range + 3
    pool = np.array([(-5, 2), (3, 3), (reach, -reach), (0, -7)], np.int16)
    pick = pool[rng.integers(0, 4, size=shape)]
    far = rng.random(shape) < 0.1
    beyond = np.where(rng.random(shape) < 0.5, reach + 1, rng.integers(reach + 1, 32768, size=shape)) * rng.choice([-1, 1], size=shape)
    a["mvx"] = np.where(far & (rng.random(shape) < 0.5), beyond, pick[..., 0])
    a["mvy"] = np.where(far & (a["mvx"] == pick[..., 0]), beyond, pick[..., 1])
    a["cost_best"] = np.where(rng.random(shape) < 1 / 7, mg.MARK, a["cost_best"] % 100000)
    return a


def list_statistics(refined, max_range, rows=(0, CH)):
    """what the lists of one picture's refined records [band CTUs, 85] show: the set of lengths, and how often each pruning condition fired"""
    lengths, fired = set(), dict(A_L=0, AR_A=0, BL_L=0, AL_L=0, AL_A=0, AL_full=0)
    reach = 4 * max_range + 3
    for i in range(refined.shape[0]):
        c = rows[0] * CW + i
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            gx, gy = (c % CW) * (1 << lvl) + bx, (c // CW) * (1 << lvl) + by
            if not mg.inside(W, H, lvl, gx, gy):
                continue
            v = []
            for nb in mg.neighbours(W, H, rows, lvl, gx, gy):
                r = None if nb is None else refined[nb[0] - rows[0] * CW, nb[1]]
                ok = r is not None and r["cost_best"] != mg.MARK and abs(int(r["mvx"])) <= reach and abs(int(r["mvy"])) <= reach
                v.append((int(r["mvx"]), int(r["mvy"])) if ok else None)
            lst = mg.build_list([None if x is None else (0,) + x for x in v], max_range)
            lengths.add(len(lst))
            fired["A_L"] += v[1] is not None and v[1] == v[0]
            fired["AR_A"] += v[2] is not None and v[2] == v[1]
            fired["BL_L"] += v[3] is not None and v[3] == v[0]
            fired["AL_L"] += v[4] is not None and v[4] == v[0]
            fired["AL_A"] += v[4] is not None and v[4] == v[1]
            fired["AL_full"] += v[4] is not None and v[4] not in (v[0], v[1]) and mg.AL not in [s for s, _ in lst]
    return lengths, fired


# ---- 1. the real chain: search -> refinement -> merge on one stream, no host synchronisation ------------------------------------------------------------

@pytest.mark.parametrize("dtype,bd", [(np.int16, 8), (np.int16, 10), (np.int16, 12), (np.uint8, 8)])
def test_real_chain_on_one_stream(oracle, torch_cuda, dtype, bd):
    """max_range 8: the MR = 8 layout; 33 and 64: the MR = 64 layout with a part of its window and with the whole of it staged"""
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
        found, fine, out = Guarded(torch, N * 85 * 16), Guarded(torch, N * 85 * 16), Guarded(torch, N * 85 * 16)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = st.cuda_stream
        ctx.motion_search_pu_wide_device(p, sb, stride, fstride, 2, found.ptr, None, None, stream=s, qp=qp, search_range=R)
        ctx.motion_refine_device(p, sb, stride, fstride, 2, found.ptr, fine.ptr, stream=s, qp=qp, max_range=R)
        ctx.motion_merge_device(p, sb, stride, fstride, 2, fine.ptr, out.ptr, stream=s, qp=qp, max_range=R)
        torch.cuda.synchronize()
        refined, got = fine.result(QDT, (1, N, 85)), out.result(MDT, (1, N, 85))
        mg.same(got, expected_batch(oracle, pics, bd, qp, refined, R), (dtype.__name__, bd, R))
        check_markers(got)
        ok = got["num"] > 0
        assert (got["src"][ok] != mg.ZERO).sum() > 200 and (got["num"][ok] >= 2).any()
        # where the merge wins, an inherited vector is cheaper than the node's own refined one: that is the point of the stage
        assert (got["cost_best"][ok] < refined["cost_best"][ok]).any()
    ctx.close()


# ---- 2. random refined records ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_range", [8, 33])
def test_random_refined_records(oracle, torch_cuda, max_range):
    pics = noise_pictures(60 + max_range, 3)          # noise: every candidate has its own distortion
    qp = 4                                            # bits are cheap: any list position can win
    refined = random_refined(np.random.default_rng(7 + max_range), (2, N, 85), max_range)
    ctx = capi.Context(W, H, 8, max_frames=3)
    got = run_merge(torch_cuda, ctx, np.stack(pics).astype(np.uint8), 0, W, W * H, 3, 1, refined, qp, max_range)
    mg.same(got, expected_batch(oracle, pics, 8, qp, refined, max_range), max_range)
    check_markers(got)
    lengths, fired = set(), {}
    for f in range(2):
        l, fr = list_statistics(refined[f], max_range)
        lengths |= l
        fired = {k: fired.get(k, 0) + v for k, v in fr.items()}
    assert lengths == {1, 2, 3, 4, 5} and all(v > 0 for v in fired.values()), (lengths, fired)
    ok = got["num"] > 0
    assert set(np.unique(got["src"][ok])) == {0, 1, 2, 3, 4, 5} and set(np.unique(got["idx"][ok])) == {0, 1, 2, 3, 4}
    assert set(np.unique(got["num"][ok])) == {1, 2, 3, 4, 5}
    # a vector on the limit of the reach was evaluated
    reach = 4 * max_range + 3
    assert ((got["mvx"] == reach) & (got["mvy"] == -reach) & ok).any()
    ctx.close()


# ---- 3. constructed pictures: expected values known in advance ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,fx,fy,mv", mc.HALF_CASES)
def test_a_half_sample_picture_merges_at_no_distortion(oracle, bd, fx, fy, mv):
    case = mc.half_sample_case(bd, fx, fy, mv)
    (rb, org, stride), (cb, _, _) = pel(case["ref"]), pel(case["cur"])
    ctx = capi.Context(mc.HALF_W, mc.HALF_H, bd)
    got = ctx.motion_merge(cb, rb, case["refined"], org, stride, qp=mc.HALF_QP, max_range=8)
    mc.check_half_sample(got, case["q"], mg.bit_cost(1, mr.sqrt_lambda(oracle, mc.HALF_QP, bd)))
    mg.same(got, mg.expected(oracle, cb.reshape(-1), org, stride, case["ref"], mc.HALF_W, mc.HALF_H, bd, mc.HALF_QP, case["refined"], 8, planes=case["planes"]))
    ctx.close()


def two_motion_chains(torch):
    """the two-motion pair as uint8 planes through BOTH device chains -- "wide": zero-centred at range 4, merge at that range; "centred": coarse centres,
    the search and refinement around them at range 8, merge at max_range 64 --, per chain everything queued on ONE stream with no host synchronisation in
    between, the plain tree and the tree with merge at its end -> {chain: dict of results}; computed once"""
    if "chains" not in _CACHE:
        cur, ref = mc.pictures()
        w, h, qp = mc.W, mc.H, mc.QP
        d_luma = to_dev(torch, np.stack([ref, cur]))
        c = capi.Context(w, h, 8, max_frames=2)
        n = c.num_ctus
        res = {}
        for chain in ("wide", "centred"):
            cen = Guarded(torch, n * 16)
            found = [Guarded(torch, n * k * 16) for k in (85, 124, 384)]
            fine = [Guarded(torch, n * k * 16) for k in (85, 124, 384)]
            merge, shapes = Guarded(torch, n * 85 * 16), Guarded(torch, n * 85 * 16)
            trees = {k: (Guarded(torch, n * 85 * 16), Guarded(torch, n * 256), Guarded(torch, n * 256)) for k in ("plain", "merged")}
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            s, p = st.cuda_stream, d_luma.data_ptr()
            if chain == "centred":
                R = mc.CENTRED_RANGE
                c.motion_centres_device(p, 1, w, w * h, 2, cen.ptr, stream=s, qp=qp, coarse_range=mc.COARSE)
                c.motion_search_pu_centred_device(p, 1, w, w * h, 2, cen.ptr, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
                c.motion_refine_pu_centred_device(p, 1, w, w * h, 2, cen.ptr, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s,
                                                  qp=qp, max_range=R)
                c.motion_merge_device(p, 1, w, w * h, 2, fine[0].ptr, merge.ptr, stream=s, qp=qp, max_range=mc.CENTRED_MERGE_RANGE)
            else:
                R = mc.RANGE
                c.motion_search_pu_wide_device(p, 1, w, w * h, 2, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
                c.motion_refine_pu_wide_device(p, 1, w, w * h, 2, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s, qp=qp,
                                               max_range=R)
                c.motion_merge_device(p, 1, w, w * h, 2, fine[0].ptr, merge.ptr, stream=s, qp=qp, max_range=R)
            c.pu_shape_select_device(fine[0].ptr, fine[1].ptr, fine[2].ptr, 1, shapes.ptr, stream=s)
            c.p_tree_select_device(shapes.ptr, 1, trees["plain"][1].ptr, trees["plain"][2].ptr, trees["plain"][0].ptr, stream=s)
            c.p_tree_select_merge_device(shapes.ptr, merge.ptr, 1, trees["merged"][1].ptr, trees["merged"][2].ptr, trees["merged"][0].ptr, stream=s)
            torch.cuda.synchronize()
            r = dict(centres=cen.result(IDT, (n,)) if chain == "centred" else None, refined=fine[0].result(QDT, (n, 85)), merge=merge.result(MDT, (n, 85)),
                     shapes=shapes.result(SDT, (n, 85)))
            if chain == "wide":
                assert cen.untouched()
            for k, (t, lo, hi) in trees.items():
                r[k] = (t.result(TDT, (n, 85)), lo.result(np.uint8, (n, 256)), hi.result(np.uint8, (n, 256)))
            res[chain] = r
        c.close()
        _CACHE["chains"] = res
    return _CACHE["chains"]


@pytest.mark.parametrize("chain", ["wide", "centred"])
def test_two_motions_through_both_chains_on_one_stream(oracle, torch_cuda, chain):
    got = two_motion_chains(torch_cuda)[chain]
    case = mc.two_motion_centred_case(oracle) if chain == "centred" else mc.two_motion_case(oracle)
    if chain == "centred":
        # the centres first: every explicit vector behind them is priced against them
        for f in ("mvx", "mvy", "cost_best"):
            assert np.array_equal(got["centres"][f], case["centres"][f]), (f, got["centres"], case["centres"])
    for f in QDT.names:
        assert np.array_equal(got["refined"][f], case["refined"]["nodes"][f]), f
    # the merge stage on the chain's own refined nodes: at the search range behind the zero-centred chain, at 64 on the centred chain's absolute vectors
    mg.same(got["merge"], case["merge"], "merge")
    for f in SDT.names:
        assert np.array_equal(got["shapes"][f], case["shapes"][f]), ("shapes", f)
    for k in ("plain", "merged"):
        tr.same(got[k][0], case[k][0], k)
        assert np.array_equal(got[k][1], case[k][1]) and np.array_equal(got[k][2], case[k][2]), k
    # the expected map and costs, known in advance
    mc.check_two_motions(got["refined"], got["merge"], *got["merged"], case["vector_cost"], case["c"])
    assert not (got["plain"][0]["flags"] & mg.MERGED).any()
    # ... and the library's host twin on the device's records
    hmin, hmax, hrec = capi.p_tree_select_merge(got["shapes"], got["merge"], mc.W, mc.H, with_tree=True)
    tr.same(hrec, got["merged"][0], "host")
    assert np.array_equal(hmin, got["merged"][1]) and np.array_equal(hmax, got["merged"][2])


# ---- 4. bands, guarded planes, large batches, streams, the host form --------------------------------------------------------------------------------------------

def banded_case():
    if "banded" not in _CACHE:
        ys = frames.pan_clip(W, H, 3, seed=12, v_structure=4, v_noise=-3)
        pics = clip_planes(ys, 10, low_bits_seed=4)
        refined = random_refined(np.random.default_rng(8), (2, N, 85), 8)
        _CACHE["banded"] = (pics, refined)
    return _CACHE["banded"]


def test_bands_between_canaries_and_an_empty_band(oracle, torch_cuda):
    torch = torch_cuda
    qp, R = 33, 8
    pics, full = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    ctx = capi.Context(W, H, 10, max_frames=3)
    whole = run_merge(torch, ctx, flat, org, stride, fs, 3, 2, full, qp, R)
    mg.same(whole, expected_batch(oracle, pics, 10, qp, full, R), "whole")
    for rows in ((1, 2), (1, 3)):
        part = band(full, rows)
        got = run_merge(torch, ctx, flat, org, stride, fs, 3, 2, part, qp, R, rows=rows)      # guards checked inside
        mg.same(got, expected_batch(oracle, pics, 10, qp, part, R, rows=rows), rows)
        # a band is a slice: its records differ from the whole picture's exactly where a candidate from the CTU row above was admitted to the whole picture's list
        differs = np.zeros(got.shape, bool)
        for f in MDT.names:
            differs |= got[f] != band(whole, rows)[f]
        above = np.zeros(got.shape, bool)
        for p in range(2):
            for i in range(part.shape[1]):
                c = rows[0] * CW + i
                for k in range(85):
                    lvl, bx, by = mr.node_geometry(k)
                    gx, gy = (c % CW) * (1 << lvl) + bx, (c // CW) * (1 << lvl) + by
                    if not mg.inside(W, H, lvl, gx, gy):
                        continue
                    nbs = mg.neighbours(W, H, (0, CH), lvl, gx, gy)
                    cands = [None if nb is None else tuple(int(full[p, nb[0], nb[1]][f]) for f in ("cost_best", "mvx", "mvy")) for nb in nbs]
                    admitted = [s for s, _ in mg.build_list(cands, R)]
                    above[p, i, k] = any(s != mg.ZERO and nbs[s][0] < rows[0] * CW for s in admitted)
        assert above.any() and np.array_equal(differs, above), (rows, int(differs.sum()), int(above.sum()))
        assert not above[:, CW:].any()           # only the band's first CTU row
    # an empty band writes nothing, launches nothing and succeeds
    d_luma, d_ref, out = to_dev(torch, flat), to_dev(torch, full), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_merge_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, d_ref.data_ptr(), out.ptr, rows=(2, 2), qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype,bd,max_range", [(np.int16, 10, 8), (np.uint8, 8, 33), (np.int16, 12, 64)])
def test_guarded_planes_poisoned_margins_odd_origin_and_stride(oracle, torch_cuda, dtype, bd, max_range):
    """nothing outside the picture is read for its value: the margins, the stride padding and the gap between frames hold poison; the origin and the
    stride are odd, so no row is aligned; the records land between canaries"""
    qp = 27
    ys = frames.pan_clip(W, H, 3, seed=9, v_structure=-4, v_noise=6)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3, shift=1, frame_gap=5, poison=77)
    assert stride % 2 == 1 and origin % 2 == 1
    refined = random_refined(np.random.default_rng(bd + max_range), (2, N, 85), max_range)
    ctx = capi.Context(W, H, bd, max_frames=3)
    got = run_merge(torch_cuda, ctx, flat, origin, stride, fstride, 3, np.dtype(dtype).itemsize, refined, qp, max_range)
    mg.same(got, expected_batch(oracle, pics, bd, qp, refined, max_range), (dtype.__name__, bd, max_range))
    check_markers(got)
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_more_ctus_than_the_persistent_grid(oracle, torch_cuda, max_range):
    """90 picture pairs of 12 CTUs = 1 080 CTUs in one launch, more than four workgroups on each of 256 CUs: two pictures alternate and the refined records
    repeat, so pair f equals pair f - 2; the first two pairs equal the restatement"""
    a, b = noise_pictures(90 + max_range, 2)
    NF = 91
    assert (NF - 1) * N > 4 * 256
    refined = random_refined(np.random.default_rng(max_range), (2, N, 85), max_range)
    ctx = capi.Context(W, H, 8, max_frames=NF)
    flat = np.stack([a, b] * (NF // 2) + [a]).astype(np.uint8)
    got = run_merge(torch_cuda, ctx, flat, 0, W, W * H, NF, 1, np.tile(refined, (NF // 2, 1, 1)), 30, max_range)
    mg.same(got[:2], expected_batch(oracle, [a, b, a], 8, 30, refined, max_range), "first pairs")
    first = got[:2].tobytes()
    for f in range(2, NF - 1, 2):
        assert got[f:f + 2].tobytes() == first, f
    ctx.close()


def test_two_streams_with_different_qps_and_ranges(oracle, torch_cuda):
    torch = torch_cuda
    pics, _ = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    calls = []
    for i, (qp, R) in enumerate(((12, 8), (47, 64), (30, 8), (22, 33))):
        refined = random_refined(np.random.default_rng(100 + i), (2, N, 85), R)
        calls.append((qp, R, refined, expected_batch(oracle, pics, 10, qp, refined, R)))
    ctx = capi.Context(W, H, 10, max_frames=3)
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_ref = [to_dev(torch, c[2]) for c in calls]
    outs = [Guarded(torch, c[2].size * 16) for c in calls]
    torch.cuda.synchronize()
    for i, (qp, R, _, _) in enumerate(calls):
        ctx.motion_merge_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, d_ref[i].data_ptr(), outs[i].ptr, stream=streams[i % 2].cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    for i, c in enumerate(calls):
        mg.same(outs[i].result(MDT, c[2].shape), c[3], i)
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_host_form_equals_device_form(torch_cuda, max_range):
    pics, full = banded_case()
    refined = random_refined(np.random.default_rng(3), (1, N, 85), max_range)
    planes = [pel(p) for p in pics[:2]]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=2)
    dev = run_merge(torch_cuda, ctx, np.stack([p[0] for p in planes]), org, stride, fs, 2, 2, refined, 25, max_range)
    host = ctx.motion_merge(planes[1][0], planes[0][0], refined[0], org, stride, qp=25, max_range=max_range)
    assert host.tobytes() == dev[0].tobytes() and (host["num"] > 0).sum() > 500
    ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    pics, full = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=3)
    d_luma, d_ref, out = to_dev(torch, np.stack([p[0] for p in planes])), to_dev(torch, full), Guarded(torch, full.size * 16)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr() + 2 * org, sb=2, stride=stride, fs=fs, nf=3, rb=0, re=CH, qp=30, R=8, ref=d_ref.data_ptr(), out=out.ptr)
    bad = [(dict(ctx=None), None), (dict(luma=None), "argument"), (dict(ref=None), "argument"), (dict(out=None), "argument"), (dict(nf=1), "layout"),
           (dict(sb=3), "layout"), (dict(stride=W - 1), "layout"), (dict(qp=-1), "qp"), (dict(qp=52), "qp"), (dict(R=0), "max_range"), (dict(R=65), "max_range"),
           (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"), (dict(sb=1), "uint8"), (dict(fs=stride), "overlap")]
    launched = ctx.stats()["kernels_launched"]
    for change, text in bad:
        a = dict(good, **change)
        rc = lib.fhevc_motion_merge_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["ref"], a["out"], None)
        assert rc == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    # the host form
    canary = np.full((N, 85), CANARY, np.uint8).repeat(16, axis=1).view(MDT)
    for change in (dict(qp=52), dict(max_range=0), dict(max_range=65)):
        res = canary.copy()
        kw = dict(dict(qp=30, max_range=8), **change)
        rc = lib.fhevc_motion_merge(ctx.h, planes[1][0].ctypes.data + 2 * org, planes[0][0].ctypes.data + 2 * org, stride, kw["qp"], kw["max_range"], full[0].ctypes.data,
                                    res.ctypes.data)
        assert rc == capi.E_INVALID and res.tobytes() == canary.tobytes(), change
    assert ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted
    a = good
    assert lib.fhevc_motion_merge_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["ref"], a["out"], None) == capi.OK
    torch.cuda.synchronize()
    assert not out.untouched()
    ctx.close()


def test_slot_19_counts_one_launch_per_call(torch_cuda):
    torch = torch_cuda
    pics, full = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=3)
    d_luma, d_ref, out = to_dev(torch, np.stack([p[0] for p in planes])), to_dev(torch, full), Guarded(torch, full.size * 16)
    torch.cuda.synchronize()
    ctx.enable_kernel_timing(True)
    for s in (7, 12, 15, 17, 19):
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls, R in ((1, 8), (2, 64), (3, 8)):
        ctx.motion_merge_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, d_ref.data_ptr(), out.ptr, qp=30, max_range=R)
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(19)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (7, 12, 15, 17))
    ctx.enable_kernel_timing(False)
    for s in (14, 16, 18, 20):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()


# ---- 5. the tree decision with merge costs ------------------------------------------------------------------------------------------------------------------------

def tree_case():
    """random records of the 200 x 136 context, two pictures, four rules, and their expected records and maps; computed once"""
    if "tree" not in _CACHE:
        rng = np.random.default_rng(811)
        shapes = tr.random_shapes(rng, 2, N)
        merge = mg.random_merge(rng, shapes)
        # only six CTUs of a picture have a 64x64 node inside: the four availability combinations are planted at four of those roots, not left to the draw
        for ctu, (s_ok, m_ok) in zip((0, 1, 2, 4), ((True, True), (True, False), (False, True), (False, False))):
            shapes["cost_best"][0, ctu, 0] = 40000 if s_ok else mg.MARK
            merge["cost_best"][0, ctu, 0] = 39000 + 700 * ctu if m_ok else mg.MARK
        rules = {"default": capi.p_tree_rule_default(), "r1": tr.random_rule(rng), "r2": tr.random_rule(rng), "r3": tr.random_rule(rng)}
        exp = {k: mg.tree_select(shapes, merge, W, H, rule=r) for k, r in rules.items()}
        _CACHE["tree"] = (shapes, merge, rules, exp)
    return _CACHE["tree"]


def run_tree(torch, ctx, shapes, merge, rule, rows=None, want=ALL, in_offset=0, merge_offset=0, map_offset=0, tree_offset=0, plain=False):
    """one call, then a synchronise -> (records, depth_min, depth_max), None for an output not asked for; guards checked, and an output that was not asked for
    stays untouched.  plain: fhevc_p_tree_select_device on the same shapes"""
    P, nb = shapes.shape[:2]
    held, mheld = at_offset(torch, shapes, in_offset), at_offset(torch, merge, merge_offset)
    dmin, dmax, tree = Guarded(torch, P * nb * 256, map_offset), Guarded(torch, P * nb * 256, map_offset), Guarded(torch, P * nb * 85 * 16, tree_offset)
    torch.cuda.synchronize()
    outs = (dmin.ptr if want[0] else None, dmax.ptr if want[1] else None, tree.ptr if want[2] else None)
    if plain:
        ctx.p_tree_select_device(held[1], P, *outs, rows=rows, rule=rule)
    else:
        ctx.p_tree_select_merge_device(held[1], mheld[1], P, *outs, rows=rows, rule=rule)
    torch.cuda.synchronize()
    for g, w in zip((dmin, dmax, tree), want):
        assert w or g.untouched()
    return (tree.result(TDT, (P, nb, 85)) if want[2] else None, dmin.result(np.uint8, (P, nb, 256)) if want[0] else None,
            dmax.result(np.uint8, (P, nb, 256)) if want[1] else None)


def same_all(got, exp, what):
    if got[0] is not None:
        tr.same(got[0], exp[0], what)
    for i, n in ((1, "depth_min"), (2, "depth_max")):
        if got[i] is not None:
            assert np.array_equal(got[i], exp[i]), (what, n, np.argwhere(got[i] != exp[i])[:5])


@pytest.fixture(scope="module")
def tree_ctx(torch_cuda):
    c = capi.Context(W, H, 8)
    yield c
    c.close()


def test_tree_with_random_shapes_and_merges(torch_cuda, tree_ctx):
    shapes, merge, rules, exp = tree_case()
    seen = mg.availability_combinations(shapes, merge, W, H)
    assert all(seen[l] == {(True, True), (True, False), (False, True), (False, False)} for l in range(4)), seen
    for rname, rule in rules.items():
        same_all(run_tree(torch_cuda, tree_ctx, shapes, merge, rule), exp[rname], rname)
        for p in range(2):
            hmin, hmax, hrec = capi.p_tree_select_merge(shapes[p], merge[p], W, H, rule, with_tree=True)
            same_all((hrec, hmin, hmax), tuple(e[p] for e in exp[rname]), ("host", rname, p))
    assert (exp["r1"][0]["flags"] & mg.MERGED).any() and not (exp["r1"][0]["flags"] & mg.MERGED).all()
    # every combination of NULL outputs
    for want in itertools.product((True, False), repeat=3):
        if any(want) and want != ALL:
            same_all(run_tree(torch_cuda, tree_ctx, shapes, merge, rules["r2"], want=want), exp["r2"], want)
    same_all(run_tree(torch_cuda, tree_ctx, shapes, merge, None), exp["default"], "rule NULL")
    # bands
    for rows in ((1, 2), (1, 3)):
        got = run_tree(torch_cuda, tree_ctx, band(shapes, rows), band(merge, rows), rules["r3"], rows=rows)
        same_all(got, tuple(band(e, rows) for e in exp["r3"]), rows)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_tree_pointers_off_their_alignment(torch_cuda, tree_ctx, offset):
    """d_shapes, d_merge and d_tree 4, 8, 12 bytes behind a 16-byte boundary, the maps 1, 2, 3 bytes: the same bytes"""
    shapes, merge, rules, exp = tree_case()
    aligned = run_tree(torch_cuda, tree_ctx, shapes, merge, rules["r1"])
    same_all(aligned, exp["r1"], "aligned")
    for kw in (dict(in_offset=4 * offset), dict(merge_offset=4 * offset), dict(tree_offset=4 * offset), dict(map_offset=offset),
               dict(in_offset=4 * offset, merge_offset=16 - 4 * offset, tree_offset=16 - 4 * offset, map_offset=offset)):
        got = run_tree(torch_cuda, tree_ctx, shapes, merge, rules["r1"], **kw)
        assert all(g.tobytes() == a.tobytes() for g, a in zip(got, aligned)), kw


def test_tree_with_all_merges_marked_is_the_plain_tree(torch_cuda, tree_ctx):
    shapes, merge, rules, _ = tree_case()
    none = merge.copy()
    none["cost_best"] = mg.MARK          # every other byte stays random
    for rname in ("default", "r2"):
        a = run_tree(torch_cuda, tree_ctx, shapes, none, rules[rname])
        b = run_tree(torch_cuda, tree_ctx, shapes, none, rules[rname], plain=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), rname
    # slot 17 times both forms, and a rejected call launches nothing
    tree_ctx.enable_kernel_timing(True)
    tree_ctx.kernel_timing(17, reset=True)
    run_tree(torch_cuda, tree_ctx, shapes, merge, None)
    assert tree_ctx.kernel_timing(17)[1] == 1 and tree_ctx.kernel_timing(19)[1] == 0
    tree_ctx.enable_kernel_timing(False)
    held, out = to_dev(torch_cuda, shapes), Guarded(torch_cuda, 2 * N * 256)
    launched = tree_ctx.stats()["kernels_launched"]
    lib = tree_ctx.lib
    for args in ((tree_ctx.h, held.data_ptr(), None, 2, 0, CH, None, out.ptr, None, None, None), (tree_ctx.h, None, held.data_ptr(), 2, 0, CH, None, out.ptr, None, None, None),
                 (tree_ctx.h, held.data_ptr(), held.data_ptr(), 2, 0, CH, None, None, None, None, None), (tree_ctx.h, held.data_ptr(), held.data_ptr(), 0, 0, CH, None, out.ptr, None, None, None),
                 (tree_ctx.h, held.data_ptr(), held.data_ptr(), 2, 0, CH + 1, None, out.ptr, None, None, None),
                 (tree_ctx.h, held.data_ptr(), held.data_ptr(), 2, 0, CH, C.byref(capi.p_tree_rule(stop_q8=[0, 65536, 0])), out.ptr, None, None, None)):
        assert lib.fhevc_p_tree_select_merge_device(*args) == capi.E_INVALID, args
    torch_cuda.cuda.synchronize()
    assert out.untouched() and tree_ctx.stats()["kernels_launched"] == launched


@pytest.mark.parametrize("coarse", [0, tc.COARSE])
def test_p_tree_merge_frame_equals_the_pieces(oracle, torch_cuda, coarse):
    """the 104 x 88 pair of tests/p_tree_cases.py through the one-call form, and through its pieces queued on one stream: zero-centred (merge at the search
    range) and centred (merge at 64)"""
    torch = torch_cuda
    cur, ref = tc.pictures()
    w, h, qp, R = tc.W, tc.H, tc.QP, tc.RANGE
    c = capi.Context(w, h, 8, max_frames=2)
    n = c.num_ctus
    d_luma = to_dev(torch, np.stack([ref, cur]))
    cen = Guarded(torch, n * 16)
    found = [Guarded(torch, n * k * 16) for k in (85, 124, 384)]
    fine = [Guarded(torch, n * k * 16) for k in (85, 124, 384)]
    merge, shapes, dmin, dmax = Guarded(torch, n * 85 * 16), Guarded(torch, n * 85 * 16), Guarded(torch, n * 256), Guarded(torch, n * 256)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, p = st.cuda_stream, d_luma.data_ptr()
    if coarse:
        c.motion_centres_device(p, 1, w, w * h, 2, cen.ptr, stream=s, qp=qp, coarse_range=coarse)
        c.motion_search_pu_centred_device(p, 1, w, w * h, 2, cen.ptr, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
        c.motion_refine_pu_centred_device(p, 1, w, w * h, 2, cen.ptr, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s, qp=qp,
                                          max_range=R)
    else:
        c.motion_search_pu_wide_device(p, 1, w, w * h, 2, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
        c.motion_refine_pu_wide_device(p, 1, w, w * h, 2, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s, qp=qp, max_range=R)
    c.motion_merge_device(p, 1, w, w * h, 2, fine[0].ptr, merge.ptr, stream=s, qp=qp, max_range=64 if coarse else R)
    c.pu_shape_select_device(fine[0].ptr, fine[1].ptr, fine[2].ptr, 1, shapes.ptr, stream=s)
    c.p_tree_select_merge_device(shapes.ptr, merge.ptr, 1, dmin.ptr, dmax.ptr, None, stream=s)
    torch.cuda.synchronize()
    pieces = dict(merge=merge.result(MDT, (n, 85)), shapes=shapes.result(SDT, (n, 85)), dmin=dmin.result(np.uint8, (n, 256)), dmax=dmax.result(np.uint8, (n, 256)))
    # the pieces' merge records against the restatement on the pieces' refined nodes (ragged 104 x 88: 64 at the centred chain's absolute vectors)
    bp, borg, bstride = pel(cur.astype(np.int64))
    mg.same(pieces["merge"], mg.expected(oracle, bp.reshape(-1), borg, bstride, ref.astype(np.int64), w, h, 8, qp, fine[0].result(QDT, (n, 85)), 64 if coarse else R),
            ("pieces", coarse))
    bc, org, stride = pel(cur)
    br, _, _ = pel(ref)
    before = c.stats()
    lo, hi, sh, me = c.p_tree_merge_frame(bc, br, org, stride, qp=qp, search_range=R, coarse_range=coarse, with_shapes=True, with_merge=True)
    assert lo.tobytes() == pieces["dmin"].tobytes() and hi.tobytes() == pieces["dmax"].tobytes()
    assert sh.tobytes() == pieces["shapes"].tobytes() and me.tobytes() == pieces["merge"].tobytes()
    assert c.stats()["bytes_d2h"] - before["bytes_d2h"] == n * (512 + 2 * 85 * 16)
    lo2, hi2 = c.p_tree_merge_frame(bc, br, org, stride, qp=qp, search_range=R, coarse_range=coarse)
    assert lo2.tobytes() == lo.tobytes() and hi2.tobytes() == hi.tobytes()
    # the merge stage is in the chain: the maps are the restatement's on these records, and some node took its merge cost
    erec, emin, emax = mg.tree_select(sh[None], me[None], w, h)
    assert np.array_equal(lo, emin[0]) and np.array_equal(hi, emax[0]) and (erec["flags"] & mg.MERGED).any()
    # the frame form rejects what fhevc_p_tree_frame rejects, before anything is launched
    launched = c.stats()["kernels_launched"]
    for change in (dict(search_range=9, coarse_range=1), dict(coarse_range=15), dict(search_range=65), dict(qp=52)):
        with pytest.raises(capi.FastHevcError):
            c.p_tree_merge_frame(bc, br, org, stride, **dict(dict(qp=qp, search_range=R, coarse_range=coarse), **change))
    assert c.stats()["kernels_launched"] == launched
    c.close()
