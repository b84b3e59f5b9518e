"""Config 4 (P slices): the zero-residual stage (k_motion_skip.hip) and the tree decision that stops at a skip (the skip instantiation of k_p_tree.hip)
on the MI355X, field by field against the Python restatement tests/motion_skip_ref.py, which tests/test_motion_skip_ref.py pins to the reference's own
transform without a GPU (and tests/test_motion_skip_quant_pin.py to its quantiser; tests/test_gpu_motion_skip_quant_pin.py compares the kernel with the
reference's recorded numbers directly).  Nothing is compared with a kernel's own output except where two launches must give the same bytes.

Pictures are 200 x 136 = 4 x 3 CTUs, ragged by 8 samples on both sides (the merge tests' picture), so the last column and row hold nodes that are not
INSIDE; the constructed cases bring their own sizes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import motion_merge_cases as mc
import motion_merge_ref as mg
import motion_refine_ref as mr
import motion_skip_ref as sk
import p_tree_ref as tr
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, clip_planes, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

W, H = 200, 136
CW, CH = 4, 3
N = CW * CH
MDT, QDT, KDT, TDT = capi.MOTION_MERGE_DTYPE, capi.MOTION_QPEL_DTYPE, capi.MOTION_SKIP_DTYPE, capi.TREE_DTYPE
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


def run_skip(torch, ctx, flat, origin, stride, fstride, nf, sample_bytes, merge, qp, max_range, rows=None, stream=None):
    """merge [nf - 1, band CTUs, 85] -> the skip records of the same shape; the output lies between canaries"""
    d_luma, d_merge = to_dev(torch, flat), to_dev(torch, merge)
    out = Guarded(torch, merge.size * 16)
    torch.cuda.synchronize()
    ctx.motion_skip_device(d_luma.data_ptr() + sample_bytes * origin, sample_bytes, stride, fstride, nf, d_merge.data_ptr(), out.ptr, rows=rows, stream=stream,
                           qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    return out.result(KDT, merge.shape)


def expected_batch(pics, bd, qp, merge, max_range, rows=None, w=W, h=H, planes=None):
    """pics: [H, W] samples per frame; merge [nf - 1, band CTUs, 85] compact over the band; planes: a list to keep the reference planes in between calls"""
    out = np.zeros(merge.shape, KDT)
    for f in range(1, len(pics)):
        if planes is not None and len(planes) < f:
            planes.append(mr.Planes(pics[f - 1], bd, max_range + 8))
        out[f - 1] = sk.expected(pics[f], pics[f - 1], w, h, bd, qp, merge[f - 1], max_range, rows=rows, planes=planes[f - 1] if planes is not None else None)
    return out


def check_invalid(got, merge, max_range):
    """exactly the nodes that are not INSIDE, are marked or lie out of reach carry the invalid record"""
    reach = 4 * max_range + 3
    for c in range(N):
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            ins = mg.inside(W, H, lvl, (c % CW) * (1 << lvl) + bx, (c // CW) * (1 << lvl) + by)
            for r, m in zip(got[:, c, k], merge[:, c, k]):
                valid = ins and m["cost_best"] != mg.MARK and abs(int(m["mvx"])) <= reach and abs(int(m["mvy"])) <= reach
                assert (tuple(r) == sk.INVALID) == (not valid) and r["pad"] == 0, (c, k, r, m)
                assert not valid or (r["nonzero"] <= (64 >> lvl) ** 2 and (r["flags"] & 2) <= 2 * (r["flags"] & 1) and (r["mvx"], r["mvy"]) == (m["mvx"], m["mvy"]))


def noise_pictures(seed, nf, bd=8):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, size=(H, W)).astype(np.int64) for _ in range(nf)]


def random_merge(rng, shape, max_range):
    """merge records of random bytes; vectors anywhere within the reach, on its limit, one record in ten beyond it (by one quarter sample, or anywhere), one
    in seven marked"""
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), MDT).reshape(shape).copy()
    reach = 4 * max_range + 3
    near = rng.integers(-reach, reach + 1, size=shape + (2,))
    edge = rng.random(shape) < 0.1
    near[edge] = rng.choice([-reach, reach], size=(int(edge.sum()), 2))
    far = rng.random(shape) < 0.1
    beyond = np.where(rng.random(shape) < 0.5, reach + 1, rng.integers(reach + 1, 32768, size=shape)) * rng.choice([-1, 1], size=shape)
    a["mvx"] = np.where(far & (rng.random(shape) < 0.5), beyond, near[..., 0])
    a["mvy"] = np.where(far & (a["mvx"] == near[..., 0]), beyond, near[..., 1])
    a["cost_best"] = np.where(rng.random(shape) < 1 / 7, mg.MARK, a["cost_best"] % 100000)
    return a


# ---- 1. the real chain: search -> refinement -> merge -> skip on one stream, no host synchronisation ----------------------------------------------------

@pytest.mark.parametrize("dtype,bd", [(np.int16, 8), (np.int16, 10), (np.int16, 12), (np.uint8, 8)])
def test_real_chain_on_one_stream(torch_cuda, dtype, bd):
    """max_range 8: the MR = 8 layout; 33 and 64: the MR = 64 layout with a part of its window and with the whole of it staged; QP 22 and 37"""
    torch = torch_cuda
    ys = frames.pan_clip(W, H, 2, seed=31 + bd, v_structure=-5, v_noise=3)
    pics = clip_planes(ys, bd, low_bits_seed=5)
    sb = np.dtype(dtype).itemsize
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, poison=None)
    ctx = capi.Context(W, H, bd, max_frames=2)
    d_luma = to_dev(torch, flat)
    p = d_luma.data_ptr() + sb * origin
    zero_seen = 0
    for R in (8, 33, 64):
        planes = []
        found, fine, merge = Guarded(torch, N * 85 * 16), Guarded(torch, N * 85 * 16), Guarded(torch, N * 85 * 16)
        outs = {qp: Guarded(torch, N * 85 * 16) for qp in (22, 37)}
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = st.cuda_stream
        ctx.motion_search_pu_wide_device(p, sb, stride, fstride, 2, found.ptr, None, None, stream=s, qp=27, search_range=R)
        ctx.motion_refine_device(p, sb, stride, fstride, 2, found.ptr, fine.ptr, stream=s, qp=27, max_range=R)
        ctx.motion_merge_device(p, sb, stride, fstride, 2, fine.ptr, merge.ptr, stream=s, qp=27, max_range=R)
        for qp, out in outs.items():
            ctx.motion_skip_device(p, sb, stride, fstride, 2, merge.ptr, out.ptr, stream=s, qp=qp, max_range=R)
        torch.cuda.synchronize()
        records = merge.result(MDT, (1, N, 85))
        for qp, out in outs.items():
            got = out.result(KDT, (1, N, 85))
            sk.same(got, expected_batch(pics, bd, qp, records, R, planes=planes), (dtype.__name__, bd, R, qp))
            check_invalid(got, records, R)
            zero_seen += int(((got["flags"] & 1) != 0).sum())
        # coef_max depends on no QP
        assert np.array_equal(outs[22].result(KDT, (1, N, 85))["coef_max"], outs[37].result(KDT, (1, N, 85))["coef_max"])
    assert zero_seen > 0
    ctx.close()


# ---- 2. random merge records ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_range", [8, 33])
def test_random_merge_records(torch_cuda, max_range):
    pics = noise_pictures(60 + max_range, 3)
    merge = random_merge(np.random.default_rng(7 + max_range), (2, N, 85), max_range)
    ctx = capi.Context(W, H, 8, max_frames=3)
    got = run_skip(torch_cuda, ctx, np.stack(pics).astype(np.uint8), 0, W, W * H, 3, 1, merge, 30, max_range)
    sk.same(got, expected_batch(pics, 8, 30, merge, max_range), max_range)
    check_invalid(got, merge, max_range)
    reach = 4 * max_range + 3
    ok = got["coef_max"] != sk.MARK
    assert (ok & (np.abs(got["mvx"]) == reach)).any() and (ok & (np.abs(got["mvy"]) == reach)).any()       # vectors on the limit of the reach were tested
    assert (~ok & (merge["cost_best"] == mg.MARK)).any() and (~ok & (np.abs(merge["mvx"].astype(np.int64)) == reach + 1)).any()
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_full_swing_checkerboards_at_12_bit(torch_cuda, max_range):
    """0 against 2^12 - 1 checkerboards, the current picture the inverse of the reference: at whole-sample vectors of even parity every residual is
    +-4095 in a checkerboard, at odd parity zero, in between the interpolation's overshoots: the intermediates see their extremes"""
    yy, xx = np.mgrid[0:H, 0:W]
    ref = np.where((xx + yy) & 1, 4095, 0).astype(np.int64)
    pics = [ref, 4095 - ref]
    rng = np.random.default_rng(12 + max_range)
    merge = random_merge(rng, (1, N, 85), max_range)
    whole = rng.random((1, N, 85)) < 0.5
    merge["mvx"] = np.where(whole, merge["mvx"] & ~3, merge["mvx"])
    merge["mvy"] = np.where(whole, merge["mvy"] & ~3, merge["mvy"])
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 12, max_frames=2)
    got = run_skip(torch_cuda, ctx, np.stack([p[0] for p in planes]), org, stride, fs, 2, 2, merge, 22, max_range)
    sk.same(got, expected_batch(pics, 12, 22, merge, max_range), max_range)
    ok = got["coef_max"] != sk.MARK
    # whole-sample vectors of odd parity predict the picture exactly; of even parity they leave the +-4095 checkerboard, whose largest coefficient is known
    checker = int(np.abs(sk.coefficients(np.where((xx[:8, :8] + yy[:8, :8]) & 1, -4095, 4095), 12)).max())
    assert (got["coef_max"][ok] == 0).any() and (got["coef_max"][0, :, 21:][ok[0, :, 21:]] == checker).any()
    # ... and a picture of 4095 against a picture of 0: every TU's DC coefficient is the largest value either stage can hold, 32 760
    flat = [np.zeros((H, W), np.int64), np.full((H, W), 4095, np.int64)]
    planes = [pel(p) for p in flat]
    still = np.zeros((1, N, 85), MDT)
    got = run_skip(torch_cuda, ctx, np.stack([p[0] for p in planes]), org, stride, fs, 2, 2, still, 22, max_range)
    sk.same(got, expected_batch(flat, 12, 22, still, max_range), ("flat", max_range))
    assert (got["coef_max"][got["coef_max"] != sk.MARK] == 32760).all()
    ctx.close()


# ---- 3. constructed pictures: expected values known in advance ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,fx,fy,mv", mc.HALF_CASES)
def test_a_half_sample_picture_leaves_no_residual(oracle, bd, fx, fy, mv):
    """every node inherits the true vector (but the first of each level, which takes the zero vector): coef_max == 0 and both bits at every QP"""
    case = mc.half_sample_case(bd, fx, fy, mv)
    (rb, org, stride), (cb, _, _) = pel(case["ref"]), pel(case["cur"])
    ctx = capi.Context(mc.HALF_W, mc.HALF_H, bd)
    merge = ctx.motion_merge(cb, rb, case["refined"], org, stride, qp=mc.HALF_QP, max_range=8)
    for qp in (0, 22, 51):
        got = ctx.motion_skip(cb, rb, merge, org, stride, qp=qp, max_range=8)
        sk.same(got, sk.expected(case["cur"], case["ref"], mc.HALF_W, mc.HALF_H, bd, qp, merge, 8, planes=case["planes"]), qp)
        inherited = (merge["src"] != mg.ZERO) & (merge["num"] > 0)
        assert inherited.sum() == 6 * 85 - 4 and (got["coef_max"][inherited] == 0).all() and (got["flags"][inherited] == 3).all()
        assert (got["level_sum"][inherited] == 0).all() and (got["nonzero"][inherited] == 0).all()
    ctx.close()


def test_two_motions_leave_a_residual_astride_the_boundary(oracle, torch_cuda):
    """CTU 1 of the two-motion pair moves with V2, its only neighbour CTU 0 with V1: its 64x64 node merges at the wrong vector (or at zero) and is far from
    zero at QP 22; CTU 2 inherits V2 and is exactly zero"""
    case = mc.two_motion_case(oracle)
    cur, ref = mc.pictures()
    ctx = capi.Context(mc.W, mc.H, 8)
    (rb, org, stride), (cb, _, _) = pel(ref), pel(cur)
    got = ctx.motion_skip(cb, rb, case["merge"], org, stride, qp=22, max_range=mc.RANGE)
    sk.same(got, sk.expected(cur.astype(np.int64), ref.astype(np.int64), mc.W, mc.H, 8, 22, case["merge"], mc.RANGE))
    assert got["flags"][1, 0] == 0 and got["nonzero"][1, 0] > 1000 and got["flags"][0, 0] == 0
    assert got["flags"][2, 0] == 3 and got["coef_max"][2, 0] == 0
    ctx.close()


@pytest.mark.parametrize("bd,d", sk.FLAT_CASES)
def test_a_flat_offset_flips_each_bit_at_the_qp_computed_in_advance(torch_cuda, bd, d):
    w, h = 192, 64                                   # one CTU row
    ref = np.full((h, w), 1 << (bd - 1), np.int64)
    pics = [ref, ref + d]
    exp = sk.flat_offset_expectation(bd, d)          # tests/test_motion_skip_ref.py: each bit flips once, inside the QP range
    merge = np.zeros((1, 3, 85), MDT)
    merge["cost_best"] = 7
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(w, h, bd, max_frames=2)
    d_luma, d_merge = to_dev(torch_cuda, np.stack([p[0] for p in planes])), to_dev(torch_cuda, merge)
    outs = [Guarded(torch_cuda, 3 * 85 * 16) for _ in range(52)]
    torch_cuda.cuda.synchronize()
    for qp in range(52):
        ctx.motion_skip_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 2, d_merge.data_ptr(), outs[qp].ptr, qp=qp, max_range=4)
    torch_cuda.cuda.synchronize()
    for qp in range(52):
        got = outs[qp].result(KDT, (3, 85))
        for k in range(85):
            lvl = tr.level(k)
            want = (1 if qp in exp[lvl][0] else 0) | (2 if qp in exp[lvl][1] else 0)
            tus = 4 if lvl == 0 else 1
            assert (got["flags"][:, k] == want).all() and (got["coef_max"][:, k] == d << (15 - bd)).all(), (qp, k, got[:, k])
            assert (got["nonzero"][:, k] == (0 if want & 1 else tus)).all(), (qp, k, got[:, k])
    ctx.close()


# ---- 4. bands, guarded planes, large batches, streams, the host form ------------------------------------------------------------------------------------------

def banded_case():
    if "banded" not in _CACHE:
        ys = frames.pan_clip(W, H, 3, seed=12, v_structure=4, v_noise=-3)
        pics = clip_planes(ys, 10, low_bits_seed=4)
        merge = random_merge(np.random.default_rng(8), (2, N, 85), 8)
        _CACHE["banded"] = (pics, merge)
    return _CACHE["banded"]


def test_bands_are_slices_and_an_empty_band(torch_cuda):
    torch = torch_cuda
    qp, R = 33, 8
    pics, full = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    ctx = capi.Context(W, H, 10, max_frames=3)
    whole = run_skip(torch, ctx, flat, org, stride, fs, 3, 2, full, qp, R)
    sk.same(whole, expected_batch(pics, 10, qp, full, R), "whole")
    for rows in ((1, 2), (1, 3), (0, 1)):
        got = run_skip(torch, ctx, flat, org, stride, fs, 3, 2, band(full, rows), qp, R, rows=rows)      # guards checked inside
        assert got.tobytes() == band(whole, rows).tobytes(), rows       # a node reads no neighbour: a band is exactly a slice
    d_luma, d_merge, out = to_dev(torch, flat), to_dev(torch, full), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_skip_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, d_merge.data_ptr(), out.ptr, rows=(2, 2), qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    ctx.close()


@pytest.mark.parametrize("dtype,bd,max_range", [(np.int16, 10, 8), (np.uint8, 8, 33), (np.int16, 12, 64)])
def test_guarded_planes_poisoned_margins_odd_origin_and_stride(torch_cuda, dtype, bd, max_range):
    """nothing outside the picture is read for its value: the margins, the stride padding and the gap between frames hold poison; the origin and the
    stride are odd, so no row is aligned; the records land between canaries"""
    ys = frames.pan_clip(W, H, 3, seed=9, v_structure=-4, v_noise=6)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3, shift=1, frame_gap=5, poison=77)
    assert stride % 2 == 1 and origin % 2 == 1
    merge = random_merge(np.random.default_rng(bd + max_range), (2, N, 85), max_range)
    ctx = capi.Context(W, H, bd, max_frames=3)
    got = run_skip(torch_cuda, ctx, flat, origin, stride, fstride, 3, np.dtype(dtype).itemsize, merge, 27, max_range)
    sk.same(got, expected_batch(pics, bd, 27, merge, max_range), (dtype.__name__, bd, max_range))
    check_invalid(got, merge, max_range)
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_more_ctus_than_the_persistent_grid(torch_cuda, max_range):
    """90 picture pairs of 12 CTUs = 1 080 CTUs in one launch, more than four workgroups on each of 256 CUs: two pictures alternate and the merge records
    repeat, so pair f equals pair f - 2; the first two pairs equal the restatement"""
    a, b = noise_pictures(90 + max_range, 2)
    NF = 91
    assert (NF - 1) * N > 4 * 256
    merge = random_merge(np.random.default_rng(max_range), (2, N, 85), max_range)
    ctx = capi.Context(W, H, 8, max_frames=NF)
    flat = np.stack([a, b] * (NF // 2) + [a]).astype(np.uint8)
    got = run_skip(torch_cuda, ctx, flat, 0, W, W * H, NF, 1, np.tile(merge, (NF // 2, 1, 1)), 30, max_range)
    sk.same(got[:2], expected_batch([a, b, a], 8, 30, merge, max_range), "first pairs")
    first = got[:2].tobytes()
    for f in range(2, NF - 1, 2):
        assert got[f:f + 2].tobytes() == first, f
    ctx.close()


def test_two_streams_with_different_qps_and_ranges(torch_cuda):
    torch = torch_cuda
    pics, _ = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    flat = np.stack([p[0] for p in planes])
    calls = []
    for i, (qp, R) in enumerate(((12, 8), (47, 64), (30, 8), (22, 33))):
        merge = random_merge(np.random.default_rng(100 + i), (2, N, 85), R)
        calls.append((qp, R, merge, expected_batch(pics, 10, qp, merge, R)))
    ctx = capi.Context(W, H, 10, max_frames=3)
    d_luma = to_dev(torch, flat)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_merge = [to_dev(torch, c[2]) for c in calls]
    outs = [Guarded(torch, c[2].size * 16) for c in calls]
    torch.cuda.synchronize()
    for i, (qp, R, _, _) in enumerate(calls):
        ctx.motion_skip_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, d_merge[i].data_ptr(), outs[i].ptr, stream=streams[i % 2].cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    for i, c in enumerate(calls):
        sk.same(outs[i].result(KDT, c[2].shape), c[3], i)
    ctx.close()


@pytest.mark.parametrize("max_range", [8, 64])
def test_host_form_equals_device_form_and_counts_what_it_moves(torch_cuda, max_range):
    pics, _ = banded_case()
    merge = random_merge(np.random.default_rng(3), (1, N, 85), max_range)
    planes = [pel(p) for p in pics[:2]]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=2)
    dev = run_skip(torch_cuda, ctx, np.stack([p[0] for p in planes]), org, stride, fs, 2, 2, merge, 25, max_range)
    before = ctx.stats()
    host = ctx.motion_skip(planes[1][0], planes[0][0], merge[0], org, stride, qp=25, max_range=max_range)
    after = ctx.stats()
    assert host.tobytes() == dev[0].tobytes() and (host["coef_max"] != sk.MARK).sum() > 400
    assert after["bytes_h2d"] - before["bytes_h2d"] == 4 * W * H + N * 85 * 16 and after["bytes_d2h"] - before["bytes_d2h"] == N * 85 * 16
    assert after["kernels_launched"] - before["kernels_launched"] == 1
    # a rejected call moves nothing
    with pytest.raises(capi.FastHevcError):
        ctx.motion_skip(planes[1][0], planes[0][0], merge[0], org, stride, qp=52, max_range=max_range)
    assert ctx.stats() == after
    ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    pics, full = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=3)
    d_luma, d_merge, out = to_dev(torch, np.stack([p[0] for p in planes])), to_dev(torch, full), Guarded(torch, full.size * 16)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr() + 2 * org, sb=2, stride=stride, fs=fs, nf=3, rb=0, re=CH, qp=30, R=8, merge=d_merge.data_ptr(), out=out.ptr)
    bad = [(dict(ctx=None), None), (dict(luma=None), "argument"), (dict(merge=None), "argument"), (dict(out=None), "argument"), (dict(nf=1), "layout"),
           (dict(sb=3), "layout"), (dict(stride=W - 1), "layout"), (dict(qp=-1), "qp"), (dict(qp=52), "qp"), (dict(R=0), "max_range"), (dict(R=65), "max_range"),
           (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"), (dict(sb=1), "uint8"), (dict(fs=stride), "overlap")]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_skip_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["R"], a["merge"], a["out"], None)
    for change, text in bad:
        assert call(dict(good, **change)) == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    canary = np.full((N, 85), CANARY, np.uint8).repeat(16, axis=1).view(KDT)
    for change in (dict(qp=52), dict(max_range=0), dict(max_range=65)):
        res = canary.copy()
        kw = dict(dict(qp=30, max_range=8), **change)
        rc = lib.fhevc_motion_skip(ctx.h, planes[1][0].ctypes.data + 2 * org, planes[0][0].ctypes.data + 2 * org, stride, kw["qp"], kw["max_range"], full[0].ctypes.data,
                                   res.ctypes.data)
        assert rc == capi.E_INVALID and res.tobytes() == canary.tobytes(), change
    assert ctx.stats()["kernels_launched"] == launched
    assert call(good) == capi.OK                  # the same call with nothing wrong is accepted
    torch.cuda.synchronize()
    assert not out.untouched()
    ctx.close()


def test_slot_23_counts_one_launch_per_call(torch_cuda):
    torch = torch_cuda
    pics, full = banded_case()
    planes = [pel(p) for p in pics]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    ctx = capi.Context(W, H, 10, max_frames=3)
    d_luma, d_merge, out = to_dev(torch, np.stack([p[0] for p in planes])), to_dev(torch, full), Guarded(torch, full.size * 16)
    torch.cuda.synchronize()
    ctx.enable_kernel_timing(True)
    for s in (7, 12, 15, 17, 19, 21, 23):
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls, R in ((1, 8), (2, 64), (3, 8)):
        ctx.motion_skip_device(d_luma.data_ptr() + 2 * org, 2, stride, fs, 3, d_merge.data_ptr(), out.ptr, qp=30, max_range=R)
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(23)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (7, 12, 15, 17, 19, 21))
    ctx.enable_kernel_timing(False)
    for s in (22, 24):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    ctx.close()


# ---- 5. the tree decision that stops at a skip ---------------------------------------------------------------------------------------------------------------

def tree_case():
    """random records of the 200 x 136 context, two pictures, four rules, and their expected records and maps per skip_mask; computed once"""
    if "tree" not in _CACHE:
        rng = np.random.default_rng(823)
        shapes = tr.random_shapes(rng, 2, N)
        merge = mg.random_merge(rng, shapes)
        skip = sk.random_skip(rng, (2, N, 85))
        # only six CTUs of a picture have a 64x64 node inside: merged roots with each flag value are planted, not left to the draw
        for ctu, f in zip((0, 1, 2, 4), (0, 1, 2, 3)):
            shapes["cost_best"][0, ctu, 0], merge["cost_best"][0, ctu, 0], skip["flags"][0, ctu, 0] = 40000, 39000, f
        rules = {"default": capi.p_tree_rule_default(), "r1": tr.random_rule(rng), "r2": tr.random_rule(rng), "r3": tr.random_rule(rng)}
        exp = {(k, m): sk.tree_select(shapes, merge, skip, m, W, H, rule=r) for k, r in rules.items() for m in range(4)}
        _CACHE["tree"] = (shapes, merge, skip, rules, exp)
    return _CACHE["tree"]


def run_tree(torch, ctx, shapes, merge, skip, mask, rule, rows=None, want=ALL, in_offset=0, merge_offset=0, skip_offset=0, map_offset=0, tree_offset=0, merged_only=False):
    """one call, then a synchronise -> (records, depth_min, depth_max), None for an output not asked for; guards checked, and an output that was not asked for
    stays untouched.  merged_only: fhevc_p_tree_select_merge_device on the same records"""
    P, nb = shapes.shape[:2]
    held, mheld, sheld = at_offset(torch, shapes, in_offset), at_offset(torch, merge, merge_offset), at_offset(torch, skip, skip_offset)
    dmin, dmax, tree = Guarded(torch, P * nb * 256, map_offset), Guarded(torch, P * nb * 256, map_offset), Guarded(torch, P * nb * 85 * 16, tree_offset)
    torch.cuda.synchronize()
    outs = (dmin.ptr if want[0] else None, dmax.ptr if want[1] else None, tree.ptr if want[2] else None)
    if merged_only:
        ctx.p_tree_select_merge_device(held[1], mheld[1], P, *outs, rows=rows, rule=rule)
    else:
        ctx.p_tree_select_skip_device(held[1], mheld[1], sheld[1], mask, P, *outs, rows=rows, rule=rule)
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


def test_tree_with_random_records_four_rules_and_every_mask(torch_cuda, tree_ctx):
    shapes, merge, skip, rules, exp = tree_case()
    merged = (exp[("default", 0)][0]["flags"] & mg.MERGED) != 0
    seen = sk.flag_coverage(skip, merged)
    assert all(seen[l] == {0, 1, 2, 3} for l in range(3)), seen
    for (rname, mask), e in exp.items():
        same_all(run_tree(torch_cuda, tree_ctx, shapes, merge, skip, mask, rules[rname]), e, (rname, mask))
    for mask in (1, 2, 3):
        f = exp[("r1", mask)][0]["flags"]
        assert (f & sk.SKIPPED).any() and not ((f & sk.SKIPPED != 0) & (f & mg.MERGED == 0)).any()
    # mask 0 is byte for byte the merge tree
    for rname in ("default", "r2"):
        a = run_tree(torch_cuda, tree_ctx, shapes, merge, skip, 0, rules[rname])
        b = run_tree(torch_cuda, tree_ctx, shapes, merge, skip, 0, rules[rname], merged_only=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), rname
    # every combination of NULL outputs
    for want in itertools.product((True, False), repeat=3):
        if any(want) and want != ALL:
            same_all(run_tree(torch_cuda, tree_ctx, shapes, merge, skip, 3, rules["r2"], want=want), exp[("r2", 3)], want)
    same_all(run_tree(torch_cuda, tree_ctx, shapes, merge, skip, 1, None), exp[("default", 1)], "rule NULL")
    # bands
    for rows in ((1, 2), (1, 3)):
        got = run_tree(torch_cuda, tree_ctx, band(shapes, rows), band(merge, rows), band(skip, rows), 2, rules["r3"], rows=rows)
        same_all(got, tuple(band(e, rows) for e in exp[("r3", 2)]), rows)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_tree_pointers_off_their_alignment(torch_cuda, tree_ctx, offset):
    """d_shapes, d_merge, d_skip and d_tree 4, 8, 12 bytes behind a 16-byte boundary, the maps 1, 2, 3 bytes: the same bytes"""
    shapes, merge, skip, rules, exp = tree_case()
    aligned = run_tree(torch_cuda, tree_ctx, shapes, merge, skip, 3, rules["r1"])
    same_all(aligned, exp[("r1", 3)], "aligned")
    for kw in (dict(in_offset=4 * offset), dict(merge_offset=4 * offset), dict(skip_offset=4 * offset), dict(tree_offset=4 * offset), dict(map_offset=offset),
               dict(in_offset=4 * offset, merge_offset=16 - 4 * offset, skip_offset=4 * offset, tree_offset=16 - 4 * offset, map_offset=offset)):
        got = run_tree(torch_cuda, tree_ctx, shapes, merge, skip, 3, rules["r1"], **kw)
        assert all(g.tobytes() == a.tobytes() for g, a in zip(got, aligned)), kw


def test_a_skipped_root_is_not_descended(torch_cuda):
    shapes, merge, skip = sk.root_skip_case()
    ctx = capi.Context(64, 64, 8)
    for mask, depth in ((0, 1), (1, 1), (2, 0), (3, 0)):
        rec, dmin, dmax = run_tree(torch_cuda, ctx, shapes, merge, skip, mask, None)
        same_all((rec, dmin, dmax), sk.tree_select(shapes, merge, skip, mask, 64, 64), mask)
        assert rec["cost_kids"][0, 0, 0] == 40 < rec["cost_own"][0, 0, 0] == 90000
        assert (dmax == depth).all() and (dmin == depth).all()
        assert rec["cost_tree"][0, 0, 0] == (90000 if depth == 0 else 40) and bool(rec["flags"][0, 0, 0] & sk.SKIPPED) == (depth == 0)
    ctx.close()


def test_tree_rejected_calls_and_slot_17(torch_cuda, tree_ctx):
    shapes, merge, skip, rules, _ = tree_case()
    tree_ctx.enable_kernel_timing(True)
    for s in (17, 19, 23):
        tree_ctx.kernel_timing(s, reset=True)
    run_tree(torch_cuda, tree_ctx, shapes, merge, skip, 3, None)
    assert tree_ctx.kernel_timing(17)[1] == 1 and tree_ctx.kernel_timing(19)[1] == 0 and tree_ctx.kernel_timing(23)[1] == 0
    tree_ctx.enable_kernel_timing(False)
    held, out = to_dev(torch_cuda, shapes), Guarded(torch_cuda, 2 * N * 256)
    launched = tree_ctx.stats()["kernels_launched"]
    lib, h, p = tree_ctx.lib, tree_ctx.h, held.data_ptr()
    for args in ((h, p, p, None, 1, 2, 0, CH, None, out.ptr, None, None, None), (h, p, None, p, 1, 2, 0, CH, None, out.ptr, None, None, None),
                 (h, None, p, p, 1, 2, 0, CH, None, out.ptr, None, None, None), (h, p, p, p, 4, 2, 0, CH, None, out.ptr, None, None, None),
                 (h, p, p, p, -1, 2, 0, CH, None, out.ptr, None, None, None), (h, p, p, p, 1, 2, 0, CH, None, None, None, None, None),
                 (h, p, p, p, 1, 0, 0, CH, None, out.ptr, None, None, None), (h, p, p, p, 1, 2, 0, CH + 1, None, out.ptr, None, None, None),
                 (h, p, p, p, 1, 2, 0, CH, C.byref(capi.p_tree_rule(stop_q8=[0, 65536, 0])), out.ptr, None, None, None)):
        assert lib.fhevc_p_tree_select_skip_device(*args) == capi.E_INVALID, args
    torch_cuda.cuda.synchronize()
    assert out.untouched() and tree_ctx.stats()["kernels_launched"] == launched
