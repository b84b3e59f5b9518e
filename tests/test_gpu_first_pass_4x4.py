"""The 4x4 first pass (fhevc_intra_first_pass_4x4, _all, _device) and the device form of the 85-node candidate lists
(fhevc_intra_first_pass_candidates_device), bit for bit against the CPU oracle: there is no tolerance anywhere in this file.

Expected values come from tests/first_pass_4x4_ref.py (fho_first_pass_node at n = 4 per valid PU, lists by a stable sort), which
tests/test_oracle_first_pass_4x4.py pins without a GPU.  Every valid PU of every picture is compared, and every invalid one must carry the edge
marks; the one exception is the 1920 x 1080 picture, where the oracle runs on the fixed sample of CTUs in CTUS_1080 (28 CTUs: the four corners,
the right-hand column, the ragged bottom row, and interior CTUs)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import first_pass_4x4_ref as ref4  # noqa: E402
from fasthevc_amd import capi, frames  # noqa: E402
from oracle import oracle_py as op  # noqa: E402

gpu = pytest.mark.gpu
CANARY = 0xA5
FAMILIES = {"texture16": frames.texture16_luma, "hetero": frames.hetero_luma, "fractal": frames.fractal_luma, "gratings": frames.gratings_luma,
            "polygon": frames.polygon_luma, "chirp": frames.chirp_luma, "deadleaves": frames.deadleaves_luma, "glyphs": frames.glyphs_luma,
            "waves": frames.waves_luma}
# 1920 x 1080 is 30 x 17 CTUs, the last row 56 samples high
CTUS_1080 = sorted({0, 29, 16 * 30, 16 * 30 + 29} | {r * 30 + 29 for r in (1, 4, 7, 10, 13, 15)} | {16 * 30 + c for c in (1, 5, 11, 17, 23, 28)} |
                   {r * 30 + c for r, c in ((1, 1), (2, 9), (3, 20), (5, 14), (6, 3), (8, 27), (9, 8), (11, 16), (12, 22), (13, 5), (14, 12), (15, 0))})
assert len(CTUS_1080) == 28
_cache = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _picture(family, W, H, bd, seed=1):
    """a synthetic family at bit depth bd, int16, the low bits populated"""
    key = ("pic", family, W, H, bd, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * seed + bd)
        y = np.asarray(FAMILIES[family](W, H, seed=seed)).astype(np.int16)
        _cache[key] = (y << (bd - 8)) | rng.integers(0, 1 << (bd - 8), size=y.shape).astype(np.int16)
    return _cache[key]


def _flat_picture(W, H, bd):
    return np.full((H, W), (1 << (bd - 1)) + 3, np.int16)


def _checkerboard(W, H, bd, cell):
    """full-swing samples: 0 and (1 << bd) - 1 in cells of `cell` samples (cell 1: every residual of every mode is near the format's limit)"""
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((yy // cell) + (xx // cell)) & 1) * ((1 << bd) - 1)).astype(np.int16)


def _expected(oracle, pic, bd, qp, ctus=None, tag=None):
    H, W = pic.shape
    key = ("exp", tag, W, H, bd, qp, None if ctus is None else tuple(ctus)) if tag is not None else None
    if key is None or key not in _cache:
        flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
        exp = ref4.expected(oracle, flat, org, stride, W, H, bd, qp, ctus)
        if key is None:
            return exp
        _cache[key] = exp
    return _cache[key]


def _same(got, exp, what):
    """structured NODE_DTYPE arrays, field by field (the doubles by their bits)"""
    for k in ("satd", "mode"):
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, (what, k, "first differences:", bad[:4].tolist(), got[k][tuple(bad[0])], exp[k][tuple(bad[0])])
    bad = np.argwhere(got["cost"].view(np.uint64) != exp["cost"].view(np.uint64))
    assert bad.size == 0, (what, "cost", "first differences:", bad[:4].tolist())


def _same_modes(got, exp, what):
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, "lists", "first differences [CTU, PU, slot]:", bad[:4].tolist(), got[tuple(bad[0][:2])].tolist(), exp[tuple(bad[0][:2])].tolist())


def _check_host(oracle, ctx, pic, bd, qp, what, ctus=None, tag=None, ks=(1, 3, 8)):
    exp = _expected(oracle, pic, bd, qp, ctus, tag)
    sel = slice(None) if ctus is None else list(ctus)
    flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=17)
    for k in ks:
        best, modes = ctx.intra_first_pass_4x4(flat, origin=org, stride=stride, qp=qp, num_candidates=k)
        _same(best[sel], exp["best"], (what, "best", k))
        _same_modes(modes[sel], exp["modes"][..., :k], (what, k))
    allm = ctx.intra_first_pass_4x4_all(flat, origin=org, stride=stride, qp=qp)
    _same(allm[sel], exp["all"], (what, "all"))
    return exp


# ---- parity: sizes, bit depths, QPs, content ---------------------------------------------------------------------------------------------------------------

PARITY = [(416, 240, 8, 0, "texture16"), (416, 240, 8, 32, "deadleaves"), (416, 240, 10, 22, "hetero"), (416, 240, 10, 51, "glyphs"),
          (416, 240, 12, 37, "fractal"), (416, 240, 12, 13, "waves"), (416, 240, 9, 27, "gratings"), (416, 240, 11, 44, "polygon"),
          (200, 100, 8, 40, "chirp"), (200, 100, 10, 7, "texture16"), (200, 100, 12, 30, "deadleaves")]


@gpu
@pytest.mark.parametrize("W,H,bd,qp,family", PARITY, ids=[f"{w}x{h}-{b}bit-qp{q}-{f}" for w, h, b, q, f in PARITY])
def test_best_all_and_lists_equal_the_oracle(oracle, W, H, bd, qp, family):
    ctx = capi.Context(W, H, bd)
    pic = _picture(family, W, H, bd)
    exp = _check_host(oracle, ctx, pic, bd, qp, (W, H, bd, qp, family))
    valid = exp["best"]["mode"] != 255
    assert valid.sum() == (W // 8) * (H // 8) * 4
    if H == 100:   # the 8x8 row the height cuts: inside the picture, and invalid
        cw = ctx.ctus_x
        assert not valid.reshape(2, cw, 16, 16)[1, :, 8:].any() and valid.reshape(2, cw, 16, 16)[1, :3, :8].all()
    assert len(np.unique(exp["best"]["mode"][valid])) >= 3
    ctx.close()


@gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_flat_picture_every_cost_ties(oracle, bd):
    W, H, qp = 200, 100, 32
    ctx = capi.Context(W, H, bd)
    exp = _check_host(oracle, ctx, _flat_picture(W, H, bd), bd, qp, ("flat", bd))
    valid = exp["best"]["mode"] != 255
    assert (exp["modes"][valid] == np.array([0, 1, 26, 2, 3, 4, 5, 6], np.uint8)).all()
    ctx.close()


@gpu
@pytest.mark.parametrize("bd", [8, 9, 10, 11, 12])
@pytest.mark.parametrize("cell", [1, 3])
def test_full_swing_samples(oracle, bd, cell):
    W, H, qp = 200, 100, 25
    ctx = capi.Context(W, H, bd)
    exp = _check_host(oracle, ctx, _checkerboard(W, H, bd, cell), bd, qp, ("checkerboard", bd, cell), ks=(8,))
    valid = exp["all"]["mode"] != 255
    assert int(exp["all"]["satd"][valid].max()) > 0
    ctx.close()


@gpu
def test_1080p_on_the_fixed_ctu_sample(oracle):
    W, H, bd, qp = 1920, 1080, 8, 32
    ctx = capi.Context(W, H, bd)
    pic = _picture("hetero", W, H, bd)
    exp = _check_host(oracle, ctx, pic, bd, qp, "1080p", ctus=CTUS_1080, tag="1080p", ks=(8,))
    mode = exp["best"]["mode"][CTUS_1080.index(16 * 30 + 29)].reshape(16, 16)
    assert (mode[:14] != 255).all() and (mode[14:] == 255).all()   # 1080 = 16 * 64 + 56: seven 8x8 rows in the last CTU row
    ctx.close()


# ---- device-resident batches ---------------------------------------------------------------------------------------------------------------------------------

class _Out:
    """nbytes of device output between two canary zones"""
    PAD = 256

    def __init__(self, torch, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * self.PAD,), CANARY, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + self.PAD

    def result(self, dtype=np.uint8):
        a = self.t.cpu().numpy()
        assert (a[:self.PAD] == CANARY).all() and (a[self.PAD + self.n:] == CANARY).all(), "written outside the stated extent"
        return a[self.PAD:self.PAD + self.n].copy().view(dtype)

    def untouched(self):
        return bool((self.t == CANARY).all().item())


def _batch(W, H, bd, nf=3):
    fams = ["texture16", "fractal", "polygon", "gratings"]
    return [_picture(fams[f % 4], W, H, bd, seed=2 + f) for f in range(nf)]


def _host_results(ctx, pics, bd, qp, k):
    out = []
    for p in pics:
        flat, org, stride, _ = frames.guarded_plane(p, bd, poison=None)
        out.append(ctx.intra_first_pass_4x4(flat, origin=org, stride=stride, qp=qp, num_candidates=k))
    return np.stack([b for b, _ in out]), np.stack([m for _, m in out])


@gpu
@pytest.mark.parametrize("bd,dtype", [(8, np.uint8), (8, np.int16), (10, np.int16), (12, np.int16)], ids=["8-uint8", "8-int16", "10-int16", "12-int16"])
def test_device_batch_bands_and_optional_outputs(oracle, torch_cuda, bd, dtype):
    torch, W, H, qp, k = torch_cuda, 416, 240, 29, 3
    ctx = capi.Context(W, H, bd, max_frames=3)
    pics = _batch(W, H, bd)
    nf, cw, chh, item = len(pics), ctx.ctus_x, ctx.ctus_y, np.dtype(dtype).itemsize
    host_best, host_modes = _host_results(ctx, pics, bd, qp, k)
    for f, p in enumerate(pics):   # the host entry point itself against the oracle, picture by picture
        exp = _expected(oracle, p, bd, qp, tag=("batch", f))
        _same(host_best[f], exp["best"], ("host", f))
        _same_modes(host_modes[f], exp["modes"][..., :k], ("host", f))
    flat, org, stride, fs = frames.guarded_plane(pics, bd, dtype, poison=23, frame_gap=5)
    planes = torch.from_numpy(flat).cuda()
    ptr = planes.data_ptr() + item * org
    for rb, re in [(0, chh), (1, 3), (2, 2), (chh - 1, chh), (0, 1)]:
        n = nf * (re - rb) * cw
        for want_best, want_modes in [(True, True), (True, False), (False, True)]:
            ob, om = _Out(torch, n * 256 * 16), _Out(torch, n * 256 * k)
            ctx.intra_first_pass_4x4_device(ptr, item, stride, fs, nf, ob.ptr if want_best else None, om.ptr if want_modes else None, rows=(rb, re), qp=qp,
                                            num_candidates=k)
            torch.cuda.synchronize()
            what = (bd, dtype.__name__, rb, re, want_best, want_modes)
            if want_best and n:
                _same(ob.result(capi.NODE_DTYPE).reshape(nf, (re - rb) * cw, 256), host_best[:, rb * cw:re * cw], what)
            else:
                assert ob.untouched(), what
            if want_modes and n:
                _same_modes(om.result().reshape(nf, (re - rb) * cw, 256, k), host_modes[:, rb * cw:re * cw], what)
            else:
                assert om.untouched(), what
    ctx.close()


def _oracle_candidates(oracle, pic, bd, qp, k):
    H, W = pic.shape
    cw, chh = frames.ctu_grid(W, H)
    flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
    sl = ref4.sqrt_lambda(oracle, qp, bd)
    out = np.zeros((cw * chh, 85, k), np.uint8)
    oracle.fho_first_pass_candidates_ctu.restype = None
    for c in range(cw * chh):
        oracle.fho_first_pass_candidates_ctu(op.ptr(flat, org), C.c_int(stride), C.c_int(W), C.c_int(H), C.c_int(c % cw), C.c_int(c // cw), C.c_int(bd),
                                             C.c_double(sl), C.c_int(k), C.c_void_p(out[c].ctypes.data))
    return out


@gpu
@pytest.mark.parametrize("bd,dtype,k", [(8, np.uint8, 8), (10, np.int16, 3), (12, np.int16, 1), (8, np.int16, 5)], ids=["8-uint8-k8", "10-int16-k3", "12-int16-k1", "8-int16-k5"])
def test_candidates_device_equals_the_host_entry_point_and_the_oracle(oracle, torch_cuda, bd, dtype, k):
    torch, W, H, qp = torch_cuda, 416, 240, 34
    ctx = capi.Context(W, H, bd, max_frames=3)
    pics = _batch(W, H, bd)
    nf, cw, chh, item = len(pics), ctx.ctus_x, ctx.ctus_y, np.dtype(dtype).itemsize
    host = []
    for p in pics:
        f1, o1, s1, _ = frames.guarded_plane(p, bd, poison=None)
        host.append(ctx.intra_first_pass_candidates(f1, origin=o1, stride=s1, qp=qp, num_candidates=k))
        assert np.array_equal(host[-1], _oracle_candidates(oracle, p, bd, qp, k)), "host entry point against the oracle"
    host = np.stack(host)
    flat, org, stride, fs = frames.guarded_plane(pics, bd, dtype, poison=29, extra_stride=3)
    planes = torch.from_numpy(flat).cuda()
    for rb, re in [(0, chh), (1, 2), (3, 3), (chh - 1, chh)]:
        n = nf * (re - rb) * cw
        om = _Out(torch, n * 85 * k)
        ctx.intra_first_pass_candidates_device(planes.data_ptr() + item * org, item, stride, fs, nf, om.ptr, rows=(rb, re), qp=qp, num_candidates=k)
        torch.cuda.synchronize()
        if n:
            got = om.result().reshape(nf, (re - rb) * cw, 85, k)
            bad = np.argwhere(got != host[:, rb * cw:re * cw])
            assert bad.size == 0, (bd, k, rb, re, "first differences [frame, CTU, node, slot]:", bad[:4].tolist())
        else:
            assert om.untouched()
    ctx.close()


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------------------------

LAYOUTS = [(np.int16, 0, 0), (np.int16, 1, 0), (np.int16, 3, 5), (np.int16, 8, 1), (np.uint8, 0, 0), (np.uint8, 1, 0), (np.uint8, 7, 3), (np.uint8, 16, 9)]


@gpu
@pytest.mark.parametrize("dtype,shift,extra", LAYOUTS, ids=[f"{np.dtype(d).name}-shift{s}-extra{e}" for d, s, e in LAYOUTS])
@pytest.mark.parametrize("W,H", [(416, 240), (200, 100)])
def test_layouts_and_poisoned_surroundings(oracle, torch_cuda, W, H, dtype, shift, extra):
    """origin and stride at aligned and odd positions (aligned vector loads and the per-sample fallback both run), margins, stride padding, the rows
    below the ragged picture and the gap between frames poisoned: same results; both outputs between canaries"""
    torch, bd, qp, k = torch_cuda, 8, 31, 8
    ctx = capi.Context(W, H, bd, max_frames=2)
    pics = _batch(W, H, bd, nf=2)
    item = np.dtype(dtype).itemsize
    flat, org, stride, fs = frames.guarded_plane(pics, bd, dtype, poison=41 + shift, shift=shift, extra_stride=extra, frame_gap=shift)
    planes = torch.from_numpy(flat).cuda()
    n = 2 * ctx.num_ctus
    ob, om, o85 = _Out(torch, n * 256 * 16), _Out(torch, n * 256 * k), _Out(torch, n * 85 * k)
    ctx.intra_first_pass_4x4_device(planes.data_ptr() + item * org, item, stride, fs, 2, ob.ptr, om.ptr, qp=qp, num_candidates=k)
    ctx.intra_first_pass_candidates_device(planes.data_ptr() + item * org, item, stride, fs, 2, o85.ptr, qp=qp, num_candidates=k)
    torch.cuda.synchronize()
    best, modes, m85 = ob.result(capi.NODE_DTYPE).reshape(2, -1, 256), om.result().reshape(2, -1, 256, k), o85.result().reshape(2, -1, 85, k)
    for f, p in enumerate(pics):
        exp = _expected(oracle, p, bd, qp, tag=("layout", f))
        _same(best[f], exp["best"], (W, H, dtype.__name__, shift, extra, f))
        _same_modes(modes[f], exp["modes"], (W, H, dtype.__name__, shift, extra, f))
        key = ("cand85", W, H, f)
        if key not in _cache:
            _cache[key] = _oracle_candidates(oracle, p, bd, qp, k)
        assert np.array_equal(m85[f], _cache[key]), (W, H, dtype.__name__, shift, extra, f, "85-node lists")
    if dtype == np.int16:   # the host entry points take the same plane: origin / stride at the same alignments
        for f, p in enumerate(pics):
            b, m = ctx.intra_first_pass_4x4(flat, origin=org + f * fs, stride=stride, qp=qp, num_candidates=k)
            _same(b, best[f], ("host", shift, extra, f))
            _same_modes(m, modes[f], ("host", shift, extra, f))
    ctx.close()


# ---- streams -------------------------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("bd,dtype", [(8, np.uint8), (10, np.int16)], ids=["8-uint8", "10-int16"])
def test_streams_give_the_same_bytes_and_two_in_flight_do_not_share(oracle, torch_cuda, bd, dtype):
    """the context's stream (NULL) with the caller on the default stream and no synchronisation in between, a caller's non-blocking stream, and two
    calls on two streams in flight at once (a bounded spin in front of each so that they meet on the device), different pictures on each: all give
    the oracle's bytes.  Shared scratch between launches would show in the last case."""
    torch, W, H, qp, k = torch_cuda, 416, 240, 36, 8
    ctx = capi.Context(W, H, bd, max_frames=1)
    pics = _batch(W, H, bd, nf=2)
    item, n = np.dtype(dtype).itemsize, ctx.num_ctus
    exp4 = [_expected(oracle, p, bd, qp, tag=("streams", f)) for f, p in enumerate(pics)]
    exp85 = [_oracle_candidates(oracle, p, bd, qp, k) for p in pics]
    dev = []
    for p in pics:
        flat, org, stride, _ = frames.guarded_plane(p, bd, dtype, poison=51)
        dev.append((flat, org, stride))
    staging = [torch.from_numpy(d[0]).cuda() for d in dev]
    planes = [torch.zeros_like(s) for s in staging]

    def calls(f, stream, outs):
        ptr = planes[f].data_ptr() + item * dev[f][1]
        ctx.intra_first_pass_4x4_device(ptr, item, dev[f][2], 0, 1, outs[0].ptr, outs[1].ptr, stream=stream, qp=qp, num_candidates=k)
        ctx.intra_first_pass_candidates_device(ptr, item, dev[f][2], 0, 1, outs[2].ptr, stream=stream, qp=qp, num_candidates=k)

    def check(f, outs, what):
        _same(outs[0].result(capi.NODE_DTYPE).reshape(n, 256), exp4[f]["best"], what)
        _same_modes(outs[1].result().reshape(n, 256, k), exp4[f]["modes"], what)
        assert np.array_equal(outs[2].result().reshape(n, 85, k), exp85[f]), (what, "85-node lists")

    def new_outs():
        return [_Out(torch, n * 256 * 16), _Out(torch, n * 256 * k), _Out(torch, n * 85 * k)]
    # warm-up (code objects), then the planes are cleared again
    for f in range(2):
        planes[f].copy_(staging[f])
        calls(f, None, new_outs())
    torch.cuda.synchronize()
    # (1) default-stream caller, library on its own blocking stream: producer | library | consumer without a synchronise in between
    outs = new_outs()
    copies = [torch.zeros_like(o.t) for o in outs]
    planes[0].zero_()
    torch.cuda._sleep(20_000_000)
    planes[0].copy_(staging[0])
    calls(0, None, outs)
    for c, o in zip(copies, outs):
        c.copy_(o.t)
    planes[0].zero_()
    torch.cuda.synchronize()
    for c, o in zip(copies, outs):
        o.t.copy_(c)
    check(0, outs, "context stream behind the default stream")
    # (2) a caller's non-blocking stream
    s = torch.cuda.Stream()
    outs = new_outs()
    planes[1].zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)
        planes[1].copy_(staging[1])
        calls(1, s.cuda_stream, outs)
    torch.cuda.synchronize()
    check(1, outs, "caller stream")
    # (3) two streams in flight at once
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    planes[0].copy_(staging[0])
    planes[1].copy_(staging[1])
    torch.cuda.synchronize()
    rounds = [(new_outs(), new_outs()) for _ in range(3)]
    for st in (A, B):
        with torch.cuda.stream(st):
            torch.cuda._sleep(40_000_000)
    for oa, obb in rounds:
        calls(0, A.cuda_stream, oa)
        calls(1, B.cuda_stream, obb)
    torch.cuda.synchronize()
    for i, (oa, obb) in enumerate(rounds):
        check(0, oa, ("two streams, A", i))
        check(1, obb, ("two streams, B", i))
    assert not np.array_equal(exp85[0], exp85[1]) and not np.array_equal(exp4[0]["modes"], exp4[1]["modes"])
    ctx.close()


# ---- rejected calls, timing, statistics ----------------------------------------------------------------------------------------------------------------------

@gpu
def test_rejected_calls_leave_the_outputs_untouched(torch_cuda):
    torch, W, H = torch_cuda, 416, 240
    ctx8, ctx10 = capi.Context(W, H, 8), capi.Context(W, H, 10)
    lib, n = ctx8.lib, ctx8.num_ctus
    plane = torch.zeros((H + 64) * 512, dtype=torch.int16, device="cuda")
    ob, om = _Out(torch, n * 256 * 16), _Out(torch, n * 256 * 8)
    p, b, m, chh = plane.data_ptr(), ob.ptr, om.ptr, ctx8.ctus_y

    def dev4(h, luma=p, sb=2, stride=512, nf=1, rb=0, re=chh, qp=32, k=8, best=b, modes=m):
        return lib.fhevc_intra_first_pass_4x4_device(h, luma, sb, stride, 0, nf, rb, re, qp, k, best, modes, None)

    def dev85(h, luma=p, sb=2, stride=512, nf=1, rb=0, re=chh, qp=32, k=8, modes=m):
        return lib.fhevc_intra_first_pass_candidates_device(h, luma, sb, stride, 0, nf, rb, re, qp, k, modes, None)
    bad = [dict(luma=None), dict(k=0), dict(k=9), dict(qp=-1), dict(qp=52), dict(stride=W - 1), dict(rb=-1), dict(re=chh + 1), dict(rb=3, re=2), dict(nf=0),
           dict(sb=4)]
    for kw in bad:
        assert dev4(ctx8.h, **kw) == capi.E_INVALID, ("4x4", kw)
        assert dev85(ctx8.h, **kw) == capi.E_INVALID, ("85", kw)
    assert dev4(ctx8.h, best=None, modes=None) == capi.E_INVALID and dev85(ctx8.h, modes=None) == capi.E_INVALID
    assert dev4(ctx10.h, sb=1) == capi.E_INVALID and dev85(ctx10.h, sb=1) == capi.E_INVALID   # uint8 planes on a context above 8 bit
    # num_candidates is ignored when no lists are asked for
    assert dev4(ctx8.h, k=0, modes=None) == capi.OK
    torch.cuda.synchronize()
    assert om.untouched() and not ob.untouched()
    ob2 = _Out(torch, n * 256 * 16)
    host = np.zeros((H, 512), np.int16)
    hb, hm = np.zeros(n * 256, capi.NODE_DTYPE), np.full(n * 256 * 8, CANARY, np.uint8)
    hb["mode"] = 77
    for args in [(None, 512, 32, 8, hb.ctypes.data, hm.ctypes.data), (host.ctypes.data, W - 1, 32, 8, hb.ctypes.data, hm.ctypes.data),
                 (host.ctypes.data, 512, 52, 8, hb.ctypes.data, hm.ctypes.data), (host.ctypes.data, 512, 32, 9, hb.ctypes.data, hm.ctypes.data),
                 (host.ctypes.data, 512, 32, 0, hb.ctypes.data, hm.ctypes.data), (host.ctypes.data, 512, 32, 8, None, None)]:
        assert lib.fhevc_intra_first_pass_4x4(ctx8.h, *args) == capi.E_INVALID, args
    for args in [(None, 512, 32, hb.ctypes.data), (host.ctypes.data, 512, 32, None), (host.ctypes.data, 512, -1, hb.ctypes.data), (host.ctypes.data, 100, 32, hb.ctypes.data)]:
        assert lib.fhevc_intra_first_pass_4x4_all(ctx8.h, *args) == capi.E_INVALID, args
    torch.cuda.synchronize()
    assert (hb["mode"] == 77).all() and (hm == CANARY).all() and ob2.untouched() and om.untouched()
    ctx8.close()
    ctx10.close()


@gpu
def test_kernel_timing_slot_6_and_launch_statistics(torch_cuda):
    torch, W, H, bd = torch_cuda, 416, 240, 8
    ctx = capi.Context(W, H, bd)
    pic = _picture("texture16", W, H, bd)
    flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
    planes = torch.from_numpy(flat).cuda()
    n = ctx.num_ctus
    ob, om, o85 = _Out(torch, n * 256 * 16), _Out(torch, n * 256 * 8), _Out(torch, n * 85 * 8)
    ctx.enable_kernel_timing(True)
    assert ctx.kernel_timing(6, reset=True)[1] == 0 and ctx.kernel_timing(2, reset=True)[1] == 0
    k0 = ctx.stats()["kernels_launched"]
    ctx.intra_first_pass_4x4_device(planes.data_ptr() + 2 * org, 2, stride, 0, 1, ob.ptr, om.ptr)
    ctx.intra_first_pass_4x4_device(planes.data_ptr() + 2 * org, 2, stride, 0, 1, ob.ptr, None)
    ctx.intra_first_pass_4x4(flat, origin=org, stride=stride)
    ctx.intra_first_pass_4x4_device(planes.data_ptr() + 2 * org, 2, stride, 0, 1, ob.ptr, om.ptr, rows=(1, 1))   # an empty band launches nothing
    ctx.intra_first_pass_candidates_device(planes.data_ptr() + 2 * org, 2, stride, 0, 1, o85.ptr)
    torch.cuda.synchronize()
    ms6, n6 = ctx.kernel_timing(6)
    ms2, n2 = ctx.kernel_timing(2)
    assert n6 == 3 and n2 == 1 and ms6 > 0.0 and ms2 > 0.0, (ms6, n6, ms2, n2)
    assert ctx.stats()["kernels_launched"] == k0 + 4
    assert ctx.kernel_timing(6, reset=True)[1] == 3 and ctx.kernel_timing(6)[1] == 0
    ctx.close()
