"""The depth kernel's high-byte requant forms (k_cnn.hip: requant4_i8_hi, chosen by build_weight_image for conv2 at shift 7 with conv3 at
shift 8) against the CPU oracle: depth maps, logits and the source Hadamard, bit for bit, in every sample layout the staging takes.
Blobs that take the high-byte instantiation, the same blobs held on the short forms (FHEVC_CNN_REQUANT=short), shifts that must fall back, and the blobs at the requant limits on both sides of 2^23, where the short form 2 steps aside and the
high-byte form does not (tests/test_requant_high_byte_model.py pins which form each blob takes)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as op
from fasthevc_amd import capi, frames, weights

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (200, 136)]   # one CTU; ragged on both edges, the width no multiple of 16: guarded and vector staging in one picture
QP = 27


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _env(monkeypatch, requant=None, **extra):
    """the library reads its switches when a context is created: only the ones a case names are set"""
    for k in ("FHEVC_CNN_REQUANT", "FHEVC_CNN_TRIO", "FHEVC_CNN_ARITH", "FHEVC_HADAMARD_FORM", "FHEVC_CNN_WG_PER_CU"):
        monkeypatch.delenv(k, raising=False)
    if requant:
        monkeypatch.setenv("FHEVC_CNN_REQUANT", requant)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _blob(name):
    if name.startswith("shifts"):
        w = weights.random_weights(11)
        w["shift"] = np.array([int(v) for v in name.split("-")[1:]], np.int32)
        return w
    layer, side = name.split("-")
    return weights.requant_limit_weights("high" if side == "high" else int(layer[-1]), over=side == "over")


def _plane(content, bd, W, H):
    """int16 Pel plane in HM's layout: hetero content shifted up to bd, or full-swing content (its darkest sample 0, its brightest 2^bd - 1)"""
    luma = np.ascontiguousarray(frames.hetero_luma(416, 240)[40:40 + H, 100:100 + W])   # (the generator's smallest picture is larger than a CTU)
    if content == "hetero":
        return frames.to_pel_plane(luma, bd)
    buf, org, stride = frames.native_pel_plane(luma, bd, seed=bd)
    m = org % stride
    assert buf[m:m + H, m:m + W].min() == 0 and buf[m:m + H, m:m + W].max() == (1 << bd) - 1
    return buf, org, stride


_REFS = {}   # (blob name, W, H, bd, content) -> the oracle's outputs: computed once, shared by the cases that run the blob under another switch


def _oracle_cached(oracle, name, w, content, bd, W, H):
    key = (name, W, H, bd, content)
    if key not in _REFS:
        buf, org, stride = _plane(content, bd, W, H)
        _REFS[key] = _oracle(oracle, w, buf, org, stride, W, H, bd)
    return _REFS[key]


def _oracle(oracle, w, buf, org, stride, W, H, bd):
    n = frames.ctu_grid(W, H)[0] * frames.ctu_grid(W, H)[1]
    depth, logits, had = np.zeros(n * 256, np.uint8), np.zeros(n * 42, np.int32), np.zeros(n, np.int32)
    oracle.fho_predict_frame(op.weights_from_arrays(w), op.ptr(buf.reshape(-1), org), stride, W, H, bd, QP, depth, C.c_void_p(logits.ctypes.data))
    oracle.fho_frame_src_hadamard(op.ptr(buf.reshape(-1), org), stride, W, H, had)
    return depth.reshape(n, 256), logits.reshape(n, 42), had


def _device(torch, ctx, plane, ptr_off, sample_bytes, stride, frame_stride, nf=1, rows=None, n=None):
    dev = torch.device("cuda:0")
    n = ctx.num_ctus if n is None else n
    d = torch.from_numpy(plane).to(dev)
    depth = torch.full((nf, n, 256), 9, dtype=torch.uint8, device=dev)
    had = torch.full((nf, n), -1, dtype=torch.int32, device=dev)
    logits = torch.full((nf, n, 42), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the fills above run on torch's stream: order them before the library call
    ctx.predict_frames_device(d.data_ptr() + ptr_off, sample_bytes, stride, frame_stride, nf, depth.data_ptr(), had.data_ptr(), logits.data_ptr(), rows=rows, qp=QP)
    torch.cuda.synchronize()
    return depth.cpu().numpy(), logits.cpu().numpy(), had.cpu().numpy()


BLOBS = ["shifts-6-7-8", "shifts-6-7-8:short", "shifts-6-8-7", "shifts-6-6-8", "conv3-high", "conv3-high:short",
         "conv2-edge", "conv2-over", "conv3-edge", "conv3-over", "conv3-edge:short", "conv3-over:short"]


@pytest.mark.parametrize("blob", BLOBS)
def test_depth_maps_logits_and_hadamard_equal_the_oracle(oracle, torch_cuda, monkeypatch, blob):
    """8 bit in int16 planes, 8 bit in uint8 planes and 10 bit, hetero and full-swing content, one CTU and a ragged picture"""
    name, _, requant = blob.partition(":")
    _env(monkeypatch, requant)
    w = _blob(name)
    for W, H in SHAPES:
        for bd in (8, 10):
            ctx = capi.Context(W, H, bd, w)
            assert ctx.cnn_arith == "i8"
            for content in ("hetero", "swing"):
                buf, org, stride = _plane(content, bd, W, H)
                exp = _oracle_cached(oracle, name, w, content, bd, W, H)
                layouts = [("int16", buf, 2 * org, 2, stride, buf.size)]
                if bd == 8:
                    m = org % stride
                    layouts.append(("uint8", np.ascontiguousarray(buf[m:m + H, m:m + W]).astype(np.uint8), 0, 1, W, W * H))
                for layout, plane, off, sb, st, fs in layouts:
                    got = _device(torch_cuda, ctx, plane, off, sb, st, fs)
                    what = (blob, W, H, bd, content, layout)
                    assert np.array_equal(got[0][0], exp[0]), what
                    assert np.array_equal(got[1][0], exp[1]), what
                    assert np.array_equal(got[2][0], exp[2]), what
                    # the random blobs' logits move with the content (the limit blobs saturate every channel by design: there the requant's form decides the logits)
                    assert not name.startswith("shifts") or len(np.unique(exp[1])) > 8, what
            ctx.close()


@pytest.mark.parametrize("requant", [None, "short"])
def test_samples_outside_8_bits_in_an_int16_plane_clamp_like_the_oracle(oracle, torch_cuda, monkeypatch, requant):
    """int16 planes declared 8 bit may hold anything: both ends of the staging clamp, in the vector path and in the guarded one (depth maps
    and logits; the source Hadamard is defined for in-range samples only)"""
    _env(monkeypatch, requant)
    W, H = 200, 136
    w = _blob("shifts-6-7-8")
    buf, org, stride = _plane("hetero", 8, W, H)
    m = org % stride
    rng = np.random.default_rng(5)
    pic = buf[m:m + H, m:m + W]
    sel = rng.integers(0, 6, size=pic.shape)
    for k, v in enumerate((-32768, -1, 256, 32767)):
        pic[sel == k] = v
    assert pic.min() == -32768 and pic.max() == 32767
    exp = _oracle(oracle, w, buf, org, stride, W, H, 8)
    ctx = capi.Context(W, H, 8, w)
    dev = torch_cuda.device("cuda:0")
    d = torch_cuda.from_numpy(buf).to(dev)
    depth = torch_cuda.full((1, ctx.num_ctus, 256), 9, dtype=torch_cuda.uint8, device=dev)
    logits = torch_cuda.full((1, ctx.num_ctus, 42), -1, dtype=torch_cuda.int32, device=dev)
    torch_cuda.cuda.synchronize()
    ctx.predict_frames_device(d.data_ptr() + 2 * org, 2, stride, buf.size, 1, depth.data_ptr(), None, logits.data_ptr(), qp=QP)
    torch_cuda.cuda.synchronize()
    assert np.array_equal(depth[0].cpu().numpy(), exp[0]) and np.array_equal(logits[0].cpu().numpy(), exp[1])
    ctx.close()


def test_device_batch_of_three_pictures_in_a_band_walks_the_persistent_loop(oracle, torch_cuda, monkeypatch):
    """3 pictures x rows [1, 9) of 15 x 10 CTUs = 360 work items on one workgroup per CU (FHEVC_CNN_WG_PER_CU=1: the grid is the number of CUs), so
    that workgroups stage a next CTU while they finish one.  Pictures 1 and 2 are picture 0 rolled by whole CTU columns: a CTU's outputs do not depend on
    where it lies, so one oracle pass over the band serves all three."""
    _env(monkeypatch, FHEVC_CNN_WG_PER_CU="1")
    W, H, NF, rows = 960, 640, 3, (1, 9)
    cw, nb = W // 64, (rows[1] - rows[0]) * (W // 64)
    w = _blob("shifts-6-7-8")
    luma = frames.hetero_luma(W, H)
    planes = np.stack([frames.to_pel_plane(np.roll(luma, 64 * f, axis=1), 8)[0] for f in range(NF)])
    buf, org, stride = frames.to_pel_plane(luma, 8)
    exp = _oracle(oracle, w, buf, org + rows[0] * 64 * stride, stride, W, (rows[1] - rows[0]) * 64, 8)
    ctx = capi.Context(W, H, 8, w, max_frames=NF)
    assert nb * NF > torch_cuda.cuda.get_device_properties(0).multi_processor_count   # more work items than workgroups
    got = _device(torch_cuda, ctx, planes, 2 * org, 2, stride, planes.shape[1] * planes.shape[2], nf=NF, rows=rows, n=nb)
    for f in range(NF):
        for k, e in enumerate(exp):
            e = np.roll(e.reshape((rows[1] - rows[0], cw) + e.shape[1:]), f, axis=1).reshape(e.shape)
            assert np.array_equal(got[k][f], e), (f, k)
    ctx.close()
