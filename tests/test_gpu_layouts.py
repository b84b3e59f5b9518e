"""What lies outside the picture rectangle, how the plane is aligned, and what lies next to the outputs must not matter.

Every entry point runs on planes from frames.guarded_plane: margins, stride padding, the gap between frames and a guard zone around
the batch are POISON (the type's limits, 2^bd, random values) instead of the zeros every other test supplies, so a dropped bounds check
reads a wrong value instead of the zero that happens to be the contract's answer.  `shift` and `extra_stride` move the origin and the
rows off 16-byte (and 4-byte) alignment, so both load paths of every kernel -- aligned vector loads and guarded scalar loads -- see
interior samples.  Device outputs live inside larger tensors with a canary pattern before and after the extent the header promises
and are pre-filled with a value no result can take: a call must write all of its extent and nothing else.

The reference of every assertion is the CPU oracle on a clean zero-margin plane of the same picture (tests/test_oracle_layouts.py
shows the oracle itself is blind to the surroundings), bit for bit.  Two poison seeds must also agree with each other, which tells
a read outside the picture (GPU differs between the seeds) from any other defect (equal, but not the oracle's)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_py as op
from fasthevc_amd import capi, frames, weights

pytestmark = pytest.mark.gpu

ZONE = 4096
SEEDS = (101, 202)
# (shift, extra_stride, frame_gap) in samples.  The first is HM's own layout (aligned rows, for uint8 at W = 200 every second row
# unaligned: stride 360); the others force the guarded scalar path for the whole picture or for part of it, the last two with a
# frame stride that is not a multiple of 8 samples, so that the alignment changes from frame to frame within one launch.
LAYOUTS = {np.int16: [(0, 0, 64), (1, 0, 0), (3, 1, 5), (4, 4, 3)], np.uint8: [(0, 0, 64), (1, 0, 0), (7, 8, 5), (8, 3, 3)]}
SAMPLES = [(8, np.int16), (8, np.uint8), (10, np.int16)]
SIZES = [(200, 136), (416, 244), (64, 8), (192, 128)]
_cache = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _canary(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 7) & 0xFF).astype(np.uint8)


class _DeviceOut:
    """`nbytes` of device output, pre-filled with `fill`, between two canary zones of one allocation"""

    def __init__(self, torch, nbytes, fill=0xA5):
        self.n, self.fill = int(nbytes), fill
        host = _canary(2 * ZONE + self.n)
        host[ZONE:ZONE + self.n] = fill
        self.host = host
        self.t = torch.from_numpy(host.copy()).cuda()
        assert self.t.data_ptr() % 64 == 0
        self.ptr = self.t.data_ptr() + ZONE

    def result(self, dtype=np.uint8):
        back = self.t.cpu().numpy()
        assert np.array_equal(back[:ZONE], self.host[:ZONE]), "the call wrote before its output"
        assert np.array_equal(back[ZONE + self.n:], self.host[ZONE + self.n:]), "the call wrote past its output"
        return back[ZONE:ZONE + self.n].copy().view(dtype)

    def untouched(self):
        return bool((self.result() == self.fill).all())


class _HostOut(_DeviceOut):
    """the same in host memory (numpy)"""

    def __init__(self, nbytes, fill=0xA5):
        self.n, self.fill = int(nbytes), fill
        self.host = _canary(2 * ZONE + self.n)
        self.host[ZONE:ZONE + self.n] = fill
        self.buf = self.host.copy()
        self.ptr = self.buf.ctypes.data + ZONE

    def result(self, dtype=np.uint8):
        assert np.array_equal(self.buf[:ZONE], self.host[:ZONE]), "the call wrote before its output"
        assert np.array_equal(self.buf[ZONE + self.n:], self.host[ZONE + self.n:]), "the call wrote past its output"
        return self.buf[ZONE:ZONE + self.n].copy().view(dtype)


def _pictures(W, H, bd, nf=3, seed=0):
    """nf pictures at bit depth bd (int16), full range in the low bits; frame 2 repeats frame 0 (the oracle is the cost of these tests)"""
    key = ("pic", W, H, bd, nf, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed * 100 + bd)
        gens = [frames.hetero_luma, frames.texture16_luma]
        pics = []
        for f in range(min(nf, 2)):
            y = gens[f](max(W, 128), max(H, 128), seed=500 + seed + f)[:H, :W].astype(np.int16)
            pics.append((y << (bd - 8)) | rng.integers(0, 1 << (bd - 8), size=y.shape).astype(np.int16))
        _cache[key] = (pics + [pics[0]])[:nf]
    return _cache[key]


def _clean(pic, bd):
    flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
    return flat, org, stride


def _valid(W, H, c):
    cw = frames.ctu_grid(W, H)[0]
    return min(64, W - (c % cw) * 64), min(64, H - (c // cw) * 64)


def _classifier_refs(oracle, wkey, w, W, H, bd, qp, ms, mt):
    """per distinct picture of _pictures: depth, logits, flags, Hadamard, and the soft ranges at margins (ms, mt): dicts of [nf, ...] arrays"""
    key = ("cls", wkey, W, H, bd, qp, ms, mt)
    if key in _cache:
        return _cache[key]
    pics = _pictures(W, H, bd)
    n = frames.ctu_grid(W, H)[0] * frames.ctu_grid(W, H)[1]
    per = []
    for pic in pics[:2]:
        flat, org, stride = _clean(pic, bd)
        depth, logits, had = np.zeros(n * 256, np.uint8), np.zeros(n * 42, np.int32), np.zeros(n, np.int32)
        if "widths" in w:
            oracle.fho_predict_frame_family(C.byref(op.family_from_arrays(w)), op.ptr(flat, org), stride, W, H, bd, qp, depth.ctypes.data, logits.ctypes.data)
        else:
            oracle.fho_predict_frame(op.weights_from_arrays(w), op.ptr(flat, org), stride, W, H, bd, qp, depth, C.c_void_p(logits.ctypes.data))
        oracle.fho_frame_src_hadamard(op.ptr(flat, org), stride, W, H, had)
        logits = logits.reshape(n, 42)
        flags = np.zeros(n, np.uint32)
        dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
        for c in range(n):
            vw, vh = _valid(W, H, c)
            flags[c] = oracle.fho_flags_from_logits(np.ascontiguousarray(logits[c]), vw, vh)
            oracle.fho_depth_range_from_logits(np.ascontiguousarray(logits[c]), vw, vh, ms, mt, dmin[c], dmax[c])
        per.append(dict(depth=depth.reshape(n, 256), logits=logits, had=had, flags=flags, dmin=dmin, dmax=dmax))
    per = (per + [per[0]])[:len(pics)]
    _cache[key] = {k: np.stack([p[k] for p in per]) for k in per[0]}
    return _cache[key]


def _upload(torch, pics, bd, dtype, layout, seed):
    shift, extra, gap = layout
    flat, org, stride, fs = frames.guarded_plane(pics, bd, dtype, extra_stride=extra, shift=shift, frame_gap=gap, poison=seed)
    t = torch.from_numpy(flat).cuda()
    assert t.data_ptr() % 64 == 0
    item = np.dtype(dtype).itemsize
    return t, t.data_ptr() + item * org, item, stride, fs


def _bands(ch):
    """(rows, name): the whole picture, the band that ends on the bottom CTU row, the band that excludes it, a middle band, an empty one"""
    out = [((ch - 1, ch), "last")]
    if ch > 1:
        out.append(((0, ch - 1), "without-last"))
    if ch > 2:
        out.append(((1, ch - 1), "middle"))
    out.append(((min(1, ch), min(1, ch)), "empty"))
    return out


# ---- the depth classifier and the source Hadamard -----------------------------------------------------------------------------------------------------

def _check_classifier_device(oracle, torch, w, wkey, W, H, bd, dtype, with_hadamard=True):
    qp, ms, mt = 30, 3000, 1500
    ref = _classifier_refs(oracle, wkey, w, W, H, bd, qp, ms, mt)
    pics = _pictures(W, H, bd)
    cw, ch = frames.ctu_grid(W, H)
    n, lib = cw * ch, capi.load_library()
    ctx = capi.Context(W, H, bd, w, max_frames=3)
    for li, layout in enumerate(LAYOUTS[dtype]):
        got = []
        for seed in SEEDS:
            nf = 1 if (li == 1 and seed == SEEDS[1]) else 3      # one single-frame call among them
            t, ptr, sb, stride, fs = _upload(torch, pics[:nf], bd, dtype, layout, seed)
            # whole pictures, all five outputs and depth_max at margins 0 / 0
            o = dict(depth=_DeviceOut(torch, nf * n * 256, 7), dmax=_DeviceOut(torch, nf * n * 256, 7), had=_DeviceOut(torch, nf * n * 4),
                     logits=_DeviceOut(torch, nf * n * 42 * 4), flags=_DeviceOut(torch, nf * n * 4))
            torch.cuda.synchronize()
            ctx._check(lib.fhevc_predict_frames_device_range(ctx.h, ptr, sb, stride, fs, nf, 0, ch, qp, 0, 0, o["depth"].ptr, o["dmax"].ptr,
                                                             o["had"].ptr if with_hadamard else None, o["logits"].ptr, o["flags"].ptr, None))
            torch.cuda.synchronize()
            what = (W, H, bd, dtype.__name__, layout, seed)
            res = dict(depth=o["depth"].result().reshape(nf, n, 256), dmax=o["dmax"].result().reshape(nf, n, 256),
                       logits=o["logits"].result(np.int32).reshape(nf, n, 42), flags=o["flags"].result(np.uint32).reshape(nf, n))
            if with_hadamard:
                res["had"] = o["had"].result(np.int32).reshape(nf, n)
            else:
                assert o["had"].untouched()
            got.append(res)
            for k, v in res.items():
                bad = np.argwhere(v != ref["depth" if k == "dmax" else k][:nf])
                assert bad.size == 0, (what, k, "first differences [frame, CTU, ...]:", bad[:4].tolist())
            # CTU-row bands with soft margins: compact output over the band, nothing beyond it
            for (rb, re), name in _bands(ch):
                bn = (re - rb) * cw
                full = nf * n if bn == 0 else nf * bn      # the empty band gets whole-picture buffers: it must leave every byte alone
                b = dict(depth=_DeviceOut(torch, full * 256, 7), dmax=_DeviceOut(torch, full * 256, 7), had=_DeviceOut(torch, full * 4),
                         logits=_DeviceOut(torch, full * 42 * 4), flags=_DeviceOut(torch, full * 4))
                torch.cuda.synchronize()
                ctx._check(lib.fhevc_predict_frames_device_range(ctx.h, ptr, sb, stride, fs, nf, rb, re, qp, ms, mt, b["depth"].ptr, b["dmax"].ptr,
                                                                 b["had"].ptr if with_hadamard else None, b["logits"].ptr, b["flags"].ptr, None))
                torch.cuda.synchronize()
                if bn == 0:
                    assert all(x.untouched() for x in b.values()), (what, "the empty band wrote something")
                    continue
                sl = slice(rb * cw, re * cw)
                assert np.array_equal(b["depth"].result().reshape(nf, bn, 256), ref["dmin"][:nf, sl]), (what, name, "depth_min")
                assert np.array_equal(b["dmax"].result().reshape(nf, bn, 256), ref["dmax"][:nf, sl]), (what, name, "depth_max")
                assert np.array_equal(b["logits"].result(np.int32).reshape(nf, bn, 42), ref["logits"][:nf, sl]), (what, name, "logits")
                if with_hadamard:
                    assert np.array_equal(b["had"].result(np.int32).reshape(nf, bn), ref["had"][:nf, sl]), (what, name, "hadamard")
                b["flags"].result()      # the canaries around the flag words (their value under margins is the depth_min map's)
            del t
        for k in got[0]:
            m = min(got[0][k].shape[0], got[1][k].shape[0])
            assert np.array_equal(got[0][k][:m], got[1][k][:m]), (W, H, bd, layout, k, "differs between two poison seeds")
    assert len(np.unique(ref["depth"])) >= 2 or W * H < 4096
    ctx.close()


@pytest.mark.parametrize("bd,dtype", SAMPLES, ids=["8-int16", "8-uint8", "10-int16"])
@pytest.mark.parametrize("W,H", SIZES)
def test_base_classifier_device_batch(oracle, torch_cuda, cnn_arith, W, H, bd, dtype):
    _check_classifier_device(oracle, torch_cuda, weights.random_weights(6), "base6", W, H, bd, dtype)


def _member(monkeypatch, member):
    monkeypatch.delenv("FHEVC_D2_REQUANT", raising=False)
    if member == "32x1":
        return weights.random_family((32, 64, 128), 1, seed=3)
    if member == "d2-blob":
        return weights.load_any(os.path.join(capi.HERE, "weights", "depthnet_family_d2.fhw"))
    if member == "23x2-general":
        monkeypatch.setenv("FHEVC_D2_REQUANT", "general")
        return weights.random_family((23, 46, 92), 2, seed=4)
    return weights.random_family((18, 36, 72), 3, seed=5)


@pytest.mark.parametrize("W,H,bd,dtype", [(200, 136, 8, np.int16), (200, 136, 8, np.uint8), (64, 8, 10, np.int16), (8, 200, 10, np.int16)],
                         ids=["200x136-8-int16", "200x136-8-uint8", "64x8-10", "8x200-10"])
@pytest.mark.parametrize("member", ["32x1", "d2-blob", "23x2-general", "18x3"])
def test_family_classifier_device_batch(oracle, torch_cuda, monkeypatch, member, W, H, bd, dtype):
    """the 32 / 64 / 128 family kernel, the fused x 2 kernel (shipped blob: short requant; random blob: general requant) and a member on the layer path"""
    _check_classifier_device(oracle, torch_cuda, _member(monkeypatch, member), member, W, H, bd, dtype)


@pytest.mark.parametrize("bd", [8, 10])
def test_fused_hadamard_is_refused_for_unaligned_planes(oracle, torch_cuda, bd):
    """256 x 192 would fuse the source Hadamard into the depth kernel (one launch); a plane whose origin, stride or frame stride is off
    16-byte alignment must take the stand-alone kernel instead (two launches), and its result is the oracle's either way."""
    torch, W, H, qp = torch_cuda, 256, 192, 30
    w = weights.random_weights(6)
    ref = _classifier_refs(oracle, "base6", w, W, H, bd, qp, 0, 0)
    pics = _pictures(W, H, bd)
    n, lib = 12, capi.load_library()
    ctx = capi.Context(W, H, bd, w, max_frames=3)
    ctx.enable_kernel_timing(True)
    cases = [(np.int16, (0, 0, 64), True), (np.int16, (1, 0, 0), False), (np.int16, (4, 0, 0), False), (np.int16, (0, 4, 0), False), (np.int16, (0, 0, 4), False)]
    if bd == 8:
        cases += [(np.uint8, (0, 0, 64), True), (np.uint8, (8, 0, 0), False), (np.uint8, (0, 8, 0), False), (np.uint8, (0, 0, 3), False)]
    for dtype, layout, fused in cases:
        t, ptr, sb, stride, fs = _upload(torch, pics, bd, dtype, layout, 7)
        depth, had = _DeviceOut(torch, 3 * n * 256, 7), _DeviceOut(torch, 3 * n * 4)
        torch.cuda.synchronize()
        k0 = ctx.stats()["kernels_launched"]
        ctx.kernel_timing(1, reset=True)
        ctx._check(lib.fhevc_predict_frames_device(ctx.h, ptr, sb, stride, fs, 3, 0, 3, qp, depth.ptr, had.ptr, None, None, None))
        torch.cuda.synchronize()
        assert ctx.stats()["kernels_launched"] - k0 == (1 if fused else 2), (dtype.__name__, layout)
        assert ctx.kernel_timing(1)[1] == (0 if fused else 1), (dtype.__name__, layout)     # launches of the stand-alone Hadamard kernel
        assert np.array_equal(had.result(np.int32).reshape(3, n), ref["had"]), (dtype.__name__, layout)
        assert np.array_equal(depth.result().reshape(3, n, 256), ref["depth"]), (dtype.__name__, layout)
    ctx.close()


@pytest.mark.parametrize("member", ["base-i8", "d2-blob"])
def test_unaligned_1080p_equals_the_aligned_run(torch_cuda, monkeypatch, member):
    """1080p, int16, origin 2 bytes off: every interior sample through the guarded path; against the aligned run of the same picture
    (which test_gpu_parity.py / test_gpu_full_size.py pin to the oracle)"""
    torch, W, H = torch_cuda, 1920, 1080
    w = weights.random_weights(6) if member == "base-i8" else _member(monkeypatch, member)
    pic = frames.hetero_luma(W, H).astype(np.int16)
    ctx = capi.Context(W, H, 8, w, arith="i8")
    n, lib = ctx.num_ctus, capi.load_library()
    out = []
    for layout, seed in (((0, 0, 0), 1), ((1, 0, 0), 2)):
        t, ptr, sb, stride, fs = _upload(torch, [pic], 8, np.int16, layout, seed)
        depth, had = _DeviceOut(torch, n * 256, 7), _DeviceOut(torch, n * 4)
        torch.cuda.synchronize()
        ctx._check(lib.fhevc_predict_frames_device(ctx.h, ptr, sb, stride, fs, 1, 0, ctx.ctus_y, 32, depth.ptr, had.ptr, None, None, None))
        torch.cuda.synchronize()
        out.append((depth.result(), had.result(np.int32)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert len(np.unique(out[0][0])) >= 3 and out[0][0].max() <= 3
    ctx.close()


def test_expand_depth_flags_writes_exactly_its_maps(oracle, torch_cuda):
    torch, W, H = torch_cuda, 200, 136
    ref = _classifier_refs(oracle, "base6", weights.random_weights(6), W, H, 8, 30, 3000, 1500)
    ctx = capi.Context(W, H, 8, weights.random_weights(6))
    for nf in (1, 3):
        flags = torch.from_numpy(ref["flags"][:nf].view(np.int32).copy()).cuda()
        out = _DeviceOut(torch, nf * 12 * 256, 7)
        torch.cuda.synchronize()
        ctx.expand_depth_flags_device(flags.data_ptr(), nf, out.ptr)
        torch.cuda.synchronize()
        assert np.array_equal(out.result().reshape(nf, 12, 256), ref["depth"][:nf]), nf
    ctx.close()


# ---- the 35-mode first pass ---------------------------------------------------------------------------------------------------------------------------

def _edge_ctus(W, H, cap=6):
    """CTUs to compare: the right-most, the bottom-most and the corner one always, then the first and a few seeded others"""
    cw, ch = frames.ctu_grid(W, H)
    n = cw * ch
    must = [n - 1, cw - 1, n - cw, 0]
    rest = [int(c) for c in np.random.default_rng(W * H).permutation(n) if c not in must]
    return sorted(set((must + rest)[:max(cap, 4)]))


def _first_pass_refs(oracle, W, H, bd, qp, ctus):
    key = ("fp", W, H, bd, qp, tuple(ctus))
    if key not in _cache:
        sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
        cw = frames.ctu_grid(W, H)[0]
        out = []
        for pic in _pictures(W, H, bd)[:2]:
            flat, org, stride = _clean(pic, bd)
            e = np.zeros((len(ctus), 85), capi.NODE_DTYPE)
            for i, c in enumerate(ctus):
                oracle.fho_first_pass_ctu(op.ptr(flat, org), stride, W, H, c % cw, c // cw, bd, sl, e[i].ctypes.data_as(C.POINTER(op.NodeCost)))
            out.append(e)
        _cache[key] = np.stack(out + [out[0]])
    return _cache[key]


@pytest.mark.parametrize("W,H,bd,dtype", [(200, 136, 8, np.int16), (200, 136, 8, np.uint8), (200, 136, 10, np.int16), (416, 244, 8, np.uint8), (416, 244, 10, np.int16),
                                          (64, 8, 8, np.int16), (8, 200, 10, np.int16), (192, 128, 8, np.uint8), (192, 128, 10, np.int16), (200, 136, 12, np.int16)])
def test_first_pass_device_batch(oracle, torch_cuda, W, H, bd, dtype):
    torch, qp = torch_cuda, 33
    cw, ch = frames.ctu_grid(W, H)
    n = cw * ch
    ctus = _edge_ctus(W, H)
    ref = _first_pass_refs(oracle, W, H, bd, qp, ctus)
    pics = _pictures(W, H, bd)
    ctx = capi.Context(W, H, bd, max_frames=3)
    for layout in LAYOUTS[dtype]:
        got = []
        for seed in SEEDS:
            t, ptr, sb, stride, fs = _upload(torch, pics, bd, dtype, layout, seed)
            out = _DeviceOut(torch, 3 * n * 85 * 16)
            torch.cuda.synchronize()
            ctx.intra_first_pass_device(ptr, sb, stride, fs, 3, out.ptr, qp=qp)
            torch.cuda.synchronize()
            nodes = out.result(capi.NODE_DTYPE).reshape(3, n, 85)
            got.append(nodes)
            for k in ("satd", "mode", "cost"):
                bad = np.argwhere(nodes[:, ctus][k] != ref[k])
                assert bad.size == 0, (W, H, bd, layout, seed, k, "[frame, index into the compared CTUs, node]", bad[:4].tolist())
            for (rb, re), name in _bands(ch):
                bn = (re - rb) * cw
                band = _DeviceOut(torch, 3 * (bn if bn else n) * 85 * 16)
                torch.cuda.synchronize()
                ctx.intra_first_pass_device(ptr, sb, stride, fs, 3, band.ptr, rows=(rb, re), qp=qp)
                torch.cuda.synchronize()
                if bn == 0:
                    assert band.untouched(), (W, H, bd, layout, "the empty band wrote something")
                else:
                    assert band.result().tobytes() == nodes[:, rb * cw:re * cw].tobytes(), (W, H, bd, layout, seed, name)
        assert got[0].tobytes() == got[1].tobytes(), (W, H, bd, layout, "differs between two poison seeds")
    ctx.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_first_pass_host_entry_points_on_a_poisoned_plane(oracle, bd):
    """fhevc_intra_first_pass_all and _candidates: every (node, mode) SATD and the candidate lists of the edge and corner CTUs, the outputs between canaries"""
    W, H, qp = 200, 136, 33
    cw, n, lib = 4, 12, capi.load_library()
    ctus = [0, 3, 8, 11]
    pic = _pictures(W, H, bd)[0]
    flat0, org0, stride0 = _clean(pic, bd)
    sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
    oracle.fho_first_pass_candidates_ctu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    sat_ref = np.full((len(ctus), 85, 35), 0xFFFFFFFF, np.uint32)
    cand_ref = np.zeros((len(ctus), 85, 8), np.uint8)
    best_ref = _first_pass_refs(oracle, W, H, bd, qp, ctus)[0]
    node, sat = op.NodeCost(), np.zeros(35, np.uint32)
    for i, c in enumerate(ctus):
        idx = 0
        for lvl in range(4):
            nn, cnt = 64 >> lvl, 1 << lvl
            for by in range(cnt):
                for bx in range(cnt):
                    x0, y0 = (c % cw) * 64 + bx * nn, (c // cw) * 64 + by * nn
                    if x0 + nn <= W and y0 + nn <= H:
                        oracle.fho_first_pass_node(op.ptr(flat0, org0), stride0, W, H, x0, y0, nn, bd, sl, C.byref(node), C.c_void_p(sat.ctypes.data))
                        sat_ref[i, idx] = sat
                    idx += 1
        oracle.fho_first_pass_candidates_ctu(op.ptr(flat0, org0), stride0, W, H, c % cw, c // cw, bd, C.c_double(sl), 8, cand_ref[i].ctypes.data)
    ctx = capi.Context(W, H, bd)
    for layout in LAYOUTS[np.int16][1:3]:
        for seed in SEEDS:
            flat, org, stride, _ = frames.guarded_plane(pic, bd, extra_stride=layout[1], shift=layout[0], poison=seed)
            best, allm, cand = _HostOut(n * 85 * 16), _HostOut(n * 85 * 35 * 16), _HostOut(n * 85 * 8)
            ctx._check(lib.fhevc_intra_first_pass_all(ctx.h, flat.ctypes.data + 2 * org, stride, qp, best.ptr, allm.ptr))
            ctx._check(lib.fhevc_intra_first_pass_candidates(ctx.h, flat.ctypes.data + 2 * org, stride, qp, 8, cand.ptr))
            b, a = best.result(capi.NODE_DTYPE).reshape(n, 85), allm.result(capi.NODE_DTYPE).reshape(n, 85, 35)
            for k in ("satd", "mode", "cost"):
                assert np.array_equal(b[ctus][k], best_ref[k]), (bd, layout, seed, k)
            assert np.array_equal(a[ctus]["satd"], sat_ref), (bd, layout, seed)
            assert np.array_equal(cand.result().reshape(n, 85, 8)[ctus], cand_ref), (bd, layout, seed)
    ctx.close()


# ---- motion search ------------------------------------------------------------------------------------------------------------------------------------

def _motion_clip(W, H, bd):
    """three pictures of a pan whose two overlaid horizontal motions and a vertical one point out of the picture at its edges"""
    key = ("clip", W, H, bd)
    if key not in _cache:
        rng = np.random.default_rng(bd)
        ys = frames.pan_clip(max(W, 64), max(H, 64), 3, seed=9, v_structure=5, v_noise=-3)
        ys = [np.roll(y, 3 * f, axis=0)[:H, :W].astype(np.int16) for f, y in enumerate(ys)]
        _cache[key] = [(y << (bd - 8)) | rng.integers(0, 1 << (bd - 8), size=y.shape).astype(np.int16) for y in ys]
    return _cache[key]


def _motion_refs(oracle, W, H, bd, qp, rng, sad, ctus):
    key = ("mot", W, H, bd, qp, rng, sad, tuple(ctus))
    if key not in _cache:
        clip = _motion_clip(W, H, bd)
        flat, org, stride, fs = frames.guarded_plane(clip, bd, poison=None)
        sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
        cw = frames.ctu_grid(W, H)[0]
        out = np.zeros((2, len(ctus), 85), capi.MOTION_DTYPE)
        for f in (1, 2):
            for i, c in enumerate(ctus):
                oracle.fho_motion_ctu_dist(op.ptr(flat, org + f * fs), stride, op.ptr(flat, org + (f - 1) * fs), stride, W, H, c % cw, c // cw, bd, rng,
                                           C.c_double(sl), int(sad), C.c_void_p(out[f - 1, i].ctypes.data))
        _cache[key] = out
    return _cache[key]


def _winners_outside(W, H, ctus, nodes):
    """valid nodes of one picture whose cheapest vector points out of the picture: the clamped coordinates decide these"""
    cw, cnt = frames.ctu_grid(W, H)[0], 0
    for i, c in enumerate(ctus):
        idx = 0
        for lvl in range(4):
            nn, k = 64 >> lvl, 1 << lvl
            for by in range(k):
                for bx in range(k):
                    m, x0, y0 = nodes[i][idx], (c % cw) * 64 + bx * nn, (c // cw) * 64 + by * nn
                    idx += 1
                    if m["cost_best"] != 0xFFFFFFFF and (x0 + m["mvx"] < 0 or x0 + nn + m["mvx"] > W or y0 + m["mvy"] < 0 or y0 + nn + m["mvy"] > H):
                        cnt += 1
    return cnt


@pytest.mark.parametrize("W,H,bd,dtype,modes", [
    (200, 136, 8, np.int16, [(False, 4), (False, 8), (True, 4), (True, 8), (True, 64), (True, 33)]),
    (200, 136, 8, np.uint8, [(False, 4), (True, 8), (True, 64), (True, 33)]),
    (200, 136, 10, np.int16, [(False, 4), (False, 8), (True, 4), (True, 8), (True, 33)]),
    (192, 128, 8, np.uint8, [(False, 8), (True, 4), (True, 33)]),
    (192, 128, 10, np.int16, [(False, 4), (True, 8)]),
    (64, 8, 8, np.int16, [(False, 4), (True, 8), (True, 33)]),
    (200, 136, 12, np.int16, [(False, 4)])])
def test_motion_search_device_batch(oracle, torch_cuda, W, H, bd, dtype, modes):
    """the packed and the wide kernels: samples outside the picture are the replicated border (coordinate clamp), never the poison around it"""
    torch, qp = torch_cuda, 35
    cw, ch = frames.ctu_grid(W, H)
    n = cw * ch
    clip = _motion_clip(W, H, bd)
    ctx = capi.Context(W, H, bd, max_frames=3)
    for sad, rng in modes:
        ctx.set_motion_distortion("sad" if sad else "satd")
        ctus = list(range(n)) if rng <= 8 else sorted({0, cw - 1, n - cw, n - 1})      # the oracle's +-64 search costs 0.15 s per CTU
        ref = _motion_refs(oracle, W, H, bd, qp, rng, sad, ctus)
        if W >= 128:
            assert _winners_outside(W, H, ctus, ref[0]) >= 8
        for layout in LAYOUTS[dtype]:
            got = []
            for seed in SEEDS:
                t, ptr, sb, stride, fs = _upload(torch, clip, bd, dtype, layout, seed)
                out = _DeviceOut(torch, 2 * n * 85 * 16)
                torch.cuda.synchronize()
                ctx.motion_search_device(ptr, sb, stride, fs, 3, out.ptr, qp=qp, search_range=rng)
                torch.cuda.synchronize()
                nodes = out.result(capi.MOTION_DTYPE).reshape(2, n, 85)
                got.append(nodes)
                for k in capi.MOTION_DTYPE.names:
                    bad = np.argwhere(nodes[:, ctus][k] != ref[k])
                    assert bad.size == 0, (W, H, bd, sad, rng, layout, seed, k, "[pair, index into the compared CTUs, node]", bad[:4].tolist())
                for (rb, re), name in _bands(ch):
                    bn = (re - rb) * cw
                    band = _DeviceOut(torch, 2 * (bn if bn else n) * 85 * 16)
                    torch.cuda.synchronize()
                    ctx.motion_search_device(ptr, sb, stride, fs, 3, band.ptr, rows=(rb, re), qp=qp, search_range=rng)
                    torch.cuda.synchronize()
                    if bn == 0:
                        assert band.untouched(), (W, H, bd, sad, rng, layout, "the empty band wrote something")
                    else:
                        assert band.result().tobytes() == nodes[:, rb * cw:re * cw].tobytes(), (W, H, bd, sad, rng, layout, seed, name)
            assert got[0].tobytes() == got[1].tobytes(), (W, H, bd, sad, rng, layout, "differs between two poison seeds")
    ctx.close()


# ---- AQ pre-analysis ----------------------------------------------------------------------------------------------------------------------------------

def _preanalyze_refs(oracle, W, H, bd, depth_layers):
    key = ("aq", W, H, bd, depth_layers)
    if key not in _cache:
        out = []
        for pic in _pictures(W, H, bd)[:2]:
            flat, org, stride = _clean(pic, bd)
            acts, avgs = [], []
            for d in range(depth_layers):
                p = 64 >> d
                a = np.zeros(((H + p - 1) // p) * ((W + p - 1) // p))
                avgs.append(oracle.fho_preanalyze_layer(op.ptr(flat, org), stride, W, H, p, a))
                acts.append(a)
            out.append((np.concatenate(acts), np.array(avgs)))
        _cache[key] = out + [out[0]]
    return _cache[key]


@pytest.mark.parametrize("W,H,bd,dtype", [(200, 136, 8, np.int16), (200, 136, 8, np.uint8), (200, 136, 10, np.int16), (416, 240, 8, np.uint8), (416, 240, 10, np.int16),
                                          (64, 8, 10, np.int16), (8, 200, 8, np.uint8), (192, 128, 8, np.int16)])
def test_preanalysis_device_batch(oracle, torch_cuda, W, H, bd, dtype):
    """all four layers; a band writes, in the whole-picture layout of fhevc_aq_parts, the parts inside its CTU rows and nothing else"""
    torch, L = torch_cuda, 4
    cw, ch = frames.ctu_grid(W, H)
    ref = _preanalyze_refs(oracle, W, H, bd, L)
    want = np.stack([r[0] for r in ref])
    pics = _pictures(W, H, bd)
    ctx = capi.Context(W, H, bd, max_frames=3)
    off = ctx.aq_layout(L)
    total = off[-1]
    assert want.shape == (3, total)
    for layout in LAYOUTS[dtype]:
        got = []
        for seed in SEEDS:
            t, ptr, sb, stride, fs = _upload(torch, pics, bd, dtype, layout, seed)
            out = _DeviceOut(torch, 3 * total * 8)
            torch.cuda.synchronize()
            ctx.preanalyze_frames_device(ptr, sb, stride, fs, 3, out.ptr, max_aq_depth=L)
            torch.cuda.synchronize()
            act = out.result(np.float64).reshape(3, total)
            got.append(act)
            assert act.tobytes() == want.tobytes(), (W, H, bd, layout, seed, np.argwhere(act != want)[:4].tolist())
            for (rb, re), name in _bands(ch):
                band = _DeviceOut(torch, 3 * total * 8)
                torch.cuda.synchronize()
                ctx.preanalyze_frames_device(ptr, sb, stride, fs, 3, band.ptr, max_aq_depth=L, rows=(rb, re))
                torch.cuda.synchronize()
                b = band.result(np.float64).reshape(3, total)
                inside = np.zeros(total, bool)
                for d in range(L):
                    p = 64 >> d
                    px, py = (W + p - 1) // p, (H + p - 1) // p
                    r0, r1 = min(py, rb * 64 // p), min(py, re * 64 // p)
                    inside[off[d] + r0 * px:off[d] + r1 * px] = True
                assert b[:, inside].tobytes() == want[:, inside].tobytes(), (W, H, bd, layout, seed, name)
                assert (b[:, ~inside].copy().view(np.uint8) == 0xA5).all(), (W, H, bd, layout, seed, name, "parts outside the band were written")
        assert got[0].tobytes() == got[1].tobytes(), (W, H, bd, layout, "differs between two poison seeds")
    ctx.close()


# ---- host entry points: the copies are under test as well ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10])
def test_single_picture_host_entry_points(oracle, bd):
    """fhevc_predict_frame, _range, fhevc_preanalyze, fhevc_motion_search on poisoned host planes, outputs between numpy canaries.  The context first
    sees a picture of maximum-value samples: the rows of its device plane below a ragged picture are never written by the copy, so stale
    or uninitialised device rows must not be read either."""
    W, H, qp, ms, mt = 200, 136, 30, 3000, 1500
    w = weights.random_weights(6)
    n, lib = 12, capi.load_library()
    ref = _classifier_refs(oracle, "base6", w, W, H, bd, qp, ms, mt)
    aq = _preanalyze_refs(oracle, W, H, bd, 4)
    pics = _pictures(W, H, bd)
    clip = _motion_clip(W, H, bd)
    ctus = list(range(n))
    ctx = capi.Context(W, H, bd, w)
    off = ctx.aq_layout(4)
    white = np.full((H, W), (1 << bd) - 1, np.int16)
    for layout in LAYOUTS[np.int16][1:3]:
        for seed in SEEDS:
            wf, wo, ws, _ = frames.guarded_plane(white, bd, extra_stride=layout[1], shift=layout[0], poison=seed + 1)
            d0, h0 = _HostOut(n * 256, 7), _HostOut(n * 4)
            ctx._check(lib.fhevc_predict_frame(ctx.h, wf.ctypes.data + 2 * wo, ws, qp, 2, d0.ptr, h0.ptr))
            for f in (0, 1):
                flat, org, stride, _ = frames.guarded_plane(pics[f], bd, extra_stride=layout[1], shift=layout[0], poison=seed)
                p = flat.ctypes.data + 2 * org
                depth, had = _HostOut(n * 256, 7), _HostOut(n * 4)
                ctx._check(lib.fhevc_predict_frame(ctx.h, p, stride, qp, 2, depth.ptr, had.ptr))
                assert np.array_equal(depth.result().reshape(n, 256), ref["depth"][f]) and np.array_equal(had.result(np.int32), ref["had"][f]), (bd, layout, seed, f)
                dmin, dmax, had2 = _HostOut(n * 256, 7), _HostOut(n * 256, 7), _HostOut(n * 4)
                ctx._check(lib.fhevc_predict_frame_range(ctx.h, p, stride, qp, 2, ms, mt, dmin.ptr, dmax.ptr, had2.ptr))
                assert np.array_equal(dmin.result().reshape(n, 256), ref["dmin"][f]) and np.array_equal(dmax.result().reshape(n, 256), ref["dmax"][f]), (bd, layout, seed, f)
                assert np.array_equal(had2.result(np.int32), ref["had"][f])
                act, avg = _HostOut(off[-1] * 8), _HostOut(4 * 8)
                ctx._check(lib.fhevc_preanalyze(ctx.h, p, stride, 4, act.ptr, avg.ptr))
                assert act.result(np.float64).tobytes() == aq[f][0].tobytes() and avg.result(np.float64).tobytes() == aq[f][1].tobytes(), (bd, layout, seed, f)
            # motion: both planes of one poisoned batch (same stride)
            flat, org, stride, fs = frames.guarded_plane(clip[:2], bd, extra_stride=layout[1], shift=layout[0], frame_gap=5, poison=seed)
            for sad, rng in ((False, 4), (True, 33)):
                ctx.set_motion_distortion("sad" if sad else "satd")
                cmp_ctus = ctus if rng <= 8 else [0, 3, 8, 11]
                mref = _motion_refs(oracle, W, H, bd, 35, rng, sad, cmp_ctus)[0]
                out = _HostOut(n * 85 * 16)
                ctx._check(lib.fhevc_motion_search(ctx.h, flat.ctypes.data + 2 * (org + fs), flat.ctypes.data + 2 * org, stride, 35, rng, out.ptr))
                nodes = out.result(capi.MOTION_DTYPE).reshape(n, 85)
                for k in capi.MOTION_DTYPE.names:
                    assert np.array_equal(nodes[cmp_ctus][k], mref[k]), (bd, layout, seed, sad, rng, k)
    ctx.close()


@pytest.mark.parametrize("bd,dtype", SAMPLES, ids=["8-int16", "8-uint8", "10-int16"])
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_batch_on_poisoned_planes(oracle, bd, dtype, pinned):
    """fhevc_predict_frames: hipMemcpy2DAsync straight from fhevc_alloc_host memory, or through the staging ring from pageable memory; 3 pictures in chunks of 2"""
    W, H, qp = 200, 136, 30
    w = weights.random_weights(6)
    n, lib = 12, capi.load_library()
    ref = _classifier_refs(oracle, "base6", w, W, H, bd, qp, 3000, 1500)
    pics = _pictures(W, H, bd)
    ctx = capi.Context(W, H, bd, w, max_frames=2)
    item = np.dtype(dtype).itemsize
    for layout in LAYOUTS[dtype][1:]:
        for seed in SEEDS:
            flat, org, stride, fs = frames.guarded_plane(pics, bd, dtype, extra_stride=layout[1], shift=layout[0], frame_gap=layout[2], poison=seed)
            src = flat
            if pinned:
                src = ctx.alloc_host(flat.shape, dtype)
                src[:] = flat
            depth, had = _HostOut(3 * n * 256, 7), _HostOut(3 * n * 4)
            ctx._check(lib.fhevc_predict_frames(ctx.h, src.ctypes.data + item * org, item, stride, fs, 3, qp, depth.ptr, had.ptr))
            assert np.array_equal(depth.result().reshape(3, n, 256), ref["depth"]), (bd, dtype.__name__, layout, seed)
            assert np.array_equal(had.result(np.int32).reshape(3, n), ref["had"]), (bd, dtype.__name__, layout, seed)
            if pinned:
                ctx.free_host(src)
    ctx.close()


def test_satd_with_poison_between_the_rows(oracle):
    """fhevc_satd on blocks cut out of poisoned buffers: strides larger than the block, odd offsets"""
    ctx = capi.Context(64, 64, 8)
    rng = np.random.default_rng(5)
    for bd in (8, 10, 12):
        for (w, h) in ((4, 4), (8, 8), (16, 4), (4, 16), (64, 64), (24, 40), (2, 2), (6, 10)):
            a = rng.integers(0, 1 << bd, size=(h, w)).astype(np.int16)
            b = rng.integers(0, 1 << bd, size=(h, w)).astype(np.int16)
            fa, oa, sa, _ = frames.guarded_plane(a, bd, margin=0, extra_stride=0, poison=None)
            fb, ob, sb_, _ = frames.guarded_plane(b, bd, margin=0, extra_stride=0, poison=None)
            exp = oracle.fho_satd(op.ptr(fa, oa), sa, op.ptr(fb, ob), sb_, w, h, bd)
            for seed in SEEDS:
                pa, poa, psa, _ = frames.guarded_plane(a, bd, margin=2, extra_stride=5, shift=1, poison=seed)
                pb, pob, psb, _ = frames.guarded_plane(b, bd, margin=1, extra_stride=0, shift=3, poison=seed + 1)
                out = C.c_uint32()
                ctx._check(ctx.lib.fhevc_satd(ctx.h, pa.ctypes.data + 2 * poa, psa, pb.ctypes.data + 2 * pob, psb, w, h, bd, C.byref(out)))
                assert out.value == exp, (bd, w, h, seed)
    ctx.close()
