"""Every kernel at bit depths 9 to 12 and on full-swing samples, against the CPU oracle bit for bit (the oracle itself is pinned to the
reference at these depths by tests/test_oracle_bit_depths.py).  9 bit is the packed 16-bit paths' other depth beside 10, 11 bit the
wide paths' other depth beside 12; the full-swing fixtures drive the packed paths' butterflies to their int16 limit, 32 (2^10 - 1),
and prove in numpy that they do before the library is called.  The blobs at the requant limits (fasthevc_amd/weights.py) check the
choice between the short and the general requant forms on both sides of 2^23."""
import ctypes as C

import numpy as np
import pytest

from oracle import bd_cases as bc
from oracle import oracle_py as op
from fasthevc_amd import capi, frames, weights

pytestmark = pytest.mark.gpu

W, H = 256, 192   # meets fhevc_cnn_can_fuse_hadamard: width a multiple of 16, height of 8, 16-byte aligned rows


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _native(bd, seed=0, content="hetero", w=W, h=H):
    luma = frames.hetero_luma(w, h, seed=4321 + seed) if content == "hetero" else frames.texture16_luma(w, h, seed=1234 + seed)
    buf, org, stride = frames.native_pel_plane(luma, bd, seed=seed * 16 + bd)
    m = org % stride
    assert buf[m:m + h, m:m + w].min() == 0 and buf[m:m + h, m:m + w].max() == (1 << bd) - 1
    return buf, org, stride


def _oracle_predict(oracle, w, buf, org, stride, bd, qp, width=W, height=H):
    n = frames.ctu_grid(width, height)[0] * frames.ctu_grid(width, height)[1]
    depth, logits, had = np.zeros(n * 256, np.uint8), np.zeros(n * 42, np.int32), np.zeros(n, np.int32)
    if "widths" in w:
        oracle.fho_predict_frame_family(C.byref(op.family_from_arrays(w)), op.ptr(buf.reshape(-1), org), stride, width, height, bd, qp,
                                        depth.ctypes.data, logits.ctypes.data)
    else:
        oracle.fho_predict_frame(op.weights_from_arrays(w), op.ptr(buf.reshape(-1), org), stride, width, height, bd, qp, depth,
                                 C.c_void_p(logits.ctypes.data))
    oracle.fho_frame_src_hadamard(op.ptr(buf.reshape(-1), org), stride, width, height, had)
    return depth.reshape(n, 256), logits.reshape(n, 42), had


def _device_logits(torch, ctx, buf, org, stride, qp):
    """predict_frames_device on the int16 plane: (depth, logits, flags) in host memory"""
    dev = torch.device("cuda:0")
    n = ctx.num_ctus
    d16 = torch.from_numpy(buf[None].copy()).to(dev)
    depth = torch.zeros((1, n, 256), dtype=torch.uint8, device=dev)
    logits = torch.zeros((1, n, 42), dtype=torch.int32, device=dev)
    flags = torch.zeros((1, n), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the fills above run on torch's stream: order them before the library call
    ctx.predict_frames_device(d16.data_ptr() + 2 * org, 2, stride, buf.size, 1, depth.data_ptr(), None, logits.data_ptr(), qp=qp,
                              d_flags=flags.data_ptr())
    torch.cuda.synchronize()
    return depth[0].cpu().numpy(), logits[0].cpu().numpy(), flags[0].cpu().numpy()


def _check_flags(oracle, logits, flags, width=W, height=H):
    cw = frames.ctu_grid(width, height)[0]
    for c in range(logits.shape[0]):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        assert int(flags[c]) & 0xFFFFFFFF == oracle.fho_flags_from_logits(np.ascontiguousarray(logits[c]), vw, vh), c


# ---- the base depth kernel -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [9, 10, 11, 12])
def test_depth_kernel_on_native_content(oracle, torch_cuda, bd, cnn_arith):
    """predict_frame (and its fused source Hadamard at 9 / 10 bit only), predict_frame_range, and the device batch's logits and flags."""
    w = weights.random_weights(3)
    buf, org, stride = _native(bd, seed=1)
    qp = 27
    exp_d, exp_l, exp_h = _oracle_predict(oracle, w, buf, org, stride, bd, qp)
    ctx = capi.Context(W, H, bd, w)
    k0 = ctx.stats()["kernels_launched"]
    d, h = ctx.predict_frame(buf, org, stride, qp=qp)
    launched = ctx.stats()["kernels_launched"] - k0
    assert np.array_equal(d, exp_d) and np.array_equal(h, exp_h)
    assert launched == (1 if bd <= 10 else 2), launched   # source Hadamard fused into the depth kernel only where the packed form holds
    dmin, dmax = ctx.predict_frame_range(buf, org, stride, qp=qp, margin=3000)
    for c in range(ctx.num_ctus):
        vw, vh = min(64, W - (c % 4) * 64), min(64, H - (c // 4) * 64)
        emin, emax = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
        oracle.fho_depth_range_from_logits(np.ascontiguousarray(exp_l[c]), vw, vh, 3000, 3000, emin, emax)
        assert np.array_equal(dmin[c], emin) and np.array_equal(dmax[c], emax), c
    dd, lg, fl = _device_logits(torch_cuda, ctx, buf, org, stride, qp)
    assert np.array_equal(dd, exp_d) and np.array_equal(lg, exp_l)
    _check_flags(oracle, lg, fl)
    ctx.close()


@pytest.mark.parametrize("bd", [9, 11])
@pytest.mark.parametrize("member", ["32x1", "23x2", "23x2-general", "18x3"])
def test_family_members_on_native_content(oracle, monkeypatch, bd, member):
    widths = {"32x1": (32, 64, 128), "23x2": (23, 46, 92), "23x2-general": (23, 46, 92), "18x3": weights.family_widths(3)}[member]
    depth = int(member.split("x")[1][0])
    if member.endswith("general"):
        monkeypatch.setenv("FHEVC_D2_REQUANT", "general")
    else:
        monkeypatch.delenv("FHEVC_D2_REQUANT", raising=False)
    f = weights.random_family(widths, depth, seed=bd)
    buf, org, stride = _native(bd, seed=2)
    exp_d, exp_l, _ = _oracle_predict(oracle, f, buf, org, stride, bd, 32)
    ctx = capi.Context(W, H, bd, f)
    d, _ = ctx.predict_frame(buf, org, stride, qp=32)
    assert np.array_equal(d, exp_d)
    ctx.close()


# ---- SATD ------------------------------------------------------------------------------------------------------------------------------------------------

def test_satd_all_shapes_and_full_swing(oracle):
    ctx = capi.Context(64, 64, 8)
    for bd in bc.SATD_BIT_DEPTHS:
        for (w, h) in bc.SATD_SHAPES:
            for rep, kind in enumerate(bc.SATD_KINDS):
                a, b = bc.satd_pair(bd, w, h, kind, rep)
                exp = oracle.fho_satd(op.ptr(a), 64, op.ptr(b), 64, w, h, bd)
                assert ctx.satd(a, b, w, h, bit_depth=bd) == exp, (bd, w, h, kind)
    ctx.close()


# ---- first pass ------------------------------------------------------------------------------------------------------------------------------------------

def _tiles(bd, invert):
    """8x8-aligned white tiles every 16 samples on a black picture (or the reverse) in CTUs 0 and 5: every neighbour of a tile is the
    background, so all 35 predictions of its 8x8 node equal the background and the residual is +-(2^bd - 1) on the whole block."""
    hi = (1 << bd) - 1
    buf, org, stride = frames.to_pel_plane(np.zeros((H, W), np.uint8), bd)
    m = org % stride
    pic = np.zeros((H, W), np.int64)
    for (cx, cy) in ((0, 0), (1, 1)):
        for ty in range(8, 64, 16):
            for tx in range(8, 64, 16):
                pic[cy * 64 + ty:cy * 64 + ty + 8, cx * 64 + tx:cx * 64 + tx + 8] = hi
    if invert:
        pic = hi - pic
    buf[m:m + H, m:m + W] = pic
    return buf, org, stride, pic


def _five_stage_peak(res):
    """largest |value| after the first five butterfly stages of the 8x8 Hadamard (three horizontal, two vertical) over the 8x8 blocks"""
    h8, h4 = bc.hadamard8(), bc.hadamard8()[:4, :4]
    v2 = np.kron(h4, np.eye(2, dtype=np.int64))   # two vertical stages: rows at distances 4 and 2 combined, 1 still apart
    peak = 0
    for y in range(0, res.shape[0] - 7, 8):
        for x in range(0, res.shape[1] - 7, 8):
            peak = max(peak, int(np.abs(v2 @ (res[y:y + 8, x:x + 8].astype(np.int64) @ h8.T)).max()))
    return peak


def _first_pass_nodes(oracle, buf, org, stride, bd, qp, ctus, width=W, height=H):
    sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
    cw = frames.ctu_grid(width, height)[0]
    exp = (op.NodeCost * 85)()
    out = {}
    for c in ctus:
        oracle.fho_first_pass_ctu(op.ptr(buf.reshape(-1), org), stride, width, height, c % cw, c // cw, bd, sl, exp)
        out[c] = np.frombuffer(exp, dtype=capi.NODE_DTYPE).copy()
    return out


def _same_nodes(got, exp, what):
    for c, e in exp.items():
        for k in ("satd", "mode", "cost"):
            assert np.array_equal(got[c][k], e[k]), (what, c, k, np.argwhere(got[c][k] != e[k])[:4].tolist())


def _oracle_all_modes(oracle, buf, org, stride, bd, qp, ctus):
    """every (node, mode) SATD of the given CTUs through fho_first_pass_node, and the candidate lists: ([len, 85, 35], [len, 85, 8])"""
    sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
    cw = frames.ctu_grid(W, H)[0]
    out = np.full((len(ctus), 85, 35), -1, np.int64)
    cand = np.zeros((len(ctus), 85, 8), np.uint8)
    best, sat = op.NodeCost(), np.zeros(35, np.uint32)
    oracle.fho_first_pass_candidates_ctu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    for i, c in enumerate(ctus):
        idx = 0
        for lvl in range(4):
            n, cnt = 64 >> lvl, 1 << lvl
            for by in range(cnt):
                for bx in range(cnt):
                    x0, y0 = (c % cw) * 64 + bx * n, (c // cw) * 64 + by * n
                    if x0 + n <= W and y0 + n <= H:
                        oracle.fho_first_pass_node(op.ptr(buf.reshape(-1), org), stride, W, H, x0, y0, n, bd, sl, C.byref(best), C.c_void_p(sat.ctypes.data))
                        out[i, idx] = sat
                    idx += 1
        oracle.fho_first_pass_candidates_ctu(C.c_void_p(buf.reshape(-1).ctypes.data + 2 * org), stride, W, H, c % cw, c // cw, bd, C.c_double(sl), 8,
                                             cand[i].ctypes.data)
    return out, cand


@pytest.mark.parametrize("bd", [9, 10, 11, 12])
def test_first_pass_full_swing_tiles(oracle, bd):
    """Packed path at 9 / 10 bit, wide at 11 / 12: best node, all 35 modes and the candidate lists over the tiled CTUs."""
    hi = (1 << bd) - 1
    ctx = capi.Context(W, H, bd)
    for invert in (False, True):
        buf, org, stride, pic = _tiles(bd, invert)
        peak = _five_stage_peak(pic - pic[0, 0])   # every prediction of a tile's 8x8 node is the background
        assert peak == 32 * hi and (bd != 10 or peak == 32 * 1023)   # at 10 bit: the packed butterflies' limit, 32 736 of int16's 32 767
        ctus = (0, 5)
        exp = _first_pass_nodes(oracle, buf, org, stride, bd, 32, ctus)
        best, allm = ctx.intra_first_pass_all(buf, org, stride, qp=32)
        _same_nodes(best, exp, (bd, invert))
        sat, cand = _oracle_all_modes(oracle, buf, org, stride, bd, 32, ctus)
        node8 = 21 + 8 + 1   # the 8x8 node of the tile at (8, 8): its residual is +-(2^bd - 1) for all 35 modes
        assert (sat[0, node8] == (((64 * hi + 2) >> 2) >> (bd - 8))).all()
        got_c = ctx.intra_first_pass_candidates(buf, org, stride, qp=32)
        for i, c in enumerate(ctus):
            assert np.array_equal(allm[c]["satd"].astype(np.int64), sat[i]), (bd, invert, c)
            assert np.array_equal(got_c[c], cand[i]), (bd, invert, c)
    ctx.close()


@pytest.mark.parametrize("bd", [9, 11])
def test_first_pass_on_native_content(oracle, bd):
    buf, org, stride = _native(bd, seed=3, content="texture16")
    ctx = capi.Context(W, H, bd)
    _same_nodes(ctx.intra_first_pass(buf, org, stride, qp=27), _first_pass_nodes(oracle, buf, org, stride, bd, 27, (0, 6, 11)), bd)
    ctx.close()


# ---- motion search ---------------------------------------------------------------------------------------------------------------------------------------

def _oracle_motion(oracle, cur, ref, origin, stride, bd, qp, rng, ctus, sad):
    cw = frames.ctu_grid(W, H)[0]
    out = {}
    sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
    cp, rp = cur.reshape(-1).ctypes.data + 2 * origin, ref.reshape(-1).ctypes.data + 2 * origin
    for c in ctus:
        o = np.zeros(85, capi.MOTION_DTYPE)
        oracle.fho_motion_ctu_dist(C.c_void_p(cp), stride, C.c_void_p(rp), stride, W, H, c % cw, c // cw, bd, rng, C.c_double(sl), 1 if sad else 0,
                                   C.c_void_p(o.ctypes.data))
        out[c] = o
    return out


def _same_motion(got, exp, what):
    for c, e in exp.items():
        for k in capi.MOTION_DTYPE.names:
            assert np.array_equal(got[c][k], e[k]), (what, c, k)


def _pan(bd, seed):
    ys = frames.pan_clip(W, H, 2, seed=seed, v_structure=5, v_noise=-3)
    (rb, org, stride), (cb, _, _) = (frames.native_pel_plane(y, bd, seed=seed + k) for k, y in enumerate(ys))
    return cb, rb, org, stride


@pytest.mark.parametrize("bd", [9, 10, 11, 12])
@pytest.mark.parametrize("sad", [False, True])
def test_motion_search_small_ranges_on_native_content(oracle, bd, sad):
    """ranges 1 .. 8: packed SATD / SAD at <= 10 bit, wide above"""
    cb, rb, org, stride = _pan(bd, 70 + bd)
    ctx = capi.Context(W, H, bd)
    if sad:
        ctx.set_motion_distortion("sad")
    for rng, qp in ((1, 22), (4, 32), (8, 37)):
        got = ctx.motion_search(cb, rb, org, stride, qp=qp, search_range=rng)
        _same_motion(got, _oracle_motion(oracle, cb, rb, org, stride, bd, qp, rng, (0, 5, 11), sad), (bd, rng, sad))
    ctx.close()


@pytest.mark.parametrize("bd", [9, 11])
def test_motion_search_wide_sad_on_native_content(oracle, bd):
    """the +-64 window above 8 bit (16-bit SAD kernel) at 9 and 11 bit"""
    cb, rb, org, stride = _pan(bd, 80 + bd)
    ctx = capi.Context(W, H, bd)
    ctx.set_motion_distortion("sad")
    got = ctx.motion_search(cb, rb, org, stride, qp=32, search_range=64)
    _same_motion(got, _oracle_motion(oracle, cb, rb, org, stride, bd, 32, 64, (0, 5), True), bd)
    ctx.close()


def _swing_planes(bd, kind):
    hi = (1 << bd) - 1
    rb, org, stride = frames.to_pel_plane(np.zeros((H, W), np.uint8), bd)
    cb = rb.copy()
    m = org % stride
    if kind == "white_black":
        cb[m:m + H, m:m + W] = hi
    elif kind == "black_white":
        rb[m:m + H, m:m + W] = hi
    else:   # half-white planes, the reference shifted by 3 samples
        cb[m:m + H, m:m + W // 2 + 4] = hi
        rb[m:m + H, m:m + W // 2 + 7] = hi
    return cb, rb, org, stride


@pytest.mark.parametrize("bd", [9, 10, 12])
@pytest.mark.parametrize("kind", ["white_black", "black_white", "half"])
def test_motion_search_full_swing(oracle, bd, kind):
    cb, rb, org, stride = _swing_planes(bd, kind)
    m = org % stride
    res = cb[m:m + 64, m:m + 64].astype(np.int64) - rb[m:m + 64, m:m + 64]
    if kind != "half":
        peak = _five_stage_peak(res)
        assert peak == 32 * ((1 << bd) - 1) and (bd != 10 or peak == 32 * 1023)
    else:   # a 3-sample strip of full-swing residual along the shifted edge
        assert _five_stage_peak(cb[m:m + 64, m + 128:m + 192].astype(np.int64) - rb[m:m + 64, m + 128:m + 192]) == 12 * ((1 << bd) - 1)
    ctx = capi.Context(W, H, bd)
    for sad, rng in ((False, 2), (False, 8), (True, 4), (True, 64)):
        ctx.set_motion_distortion("sad" if sad else "satd")
        got = ctx.motion_search(cb, rb, org, stride, qp=32, search_range=rng)
        _same_motion(got, _oracle_motion(oracle, cb, rb, org, stride, bd, 32, rng, (0, 2, 6), sad), (bd, kind, sad, rng))
    ctx.close()


# ---- AQ pre-analysis, host batch ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(len(bc.PREANALYZE_CASES)))
def test_preanalyze_at_9_to_12_bit(oracle, torch_cuda, case):
    content, w, h, bd, depth = bc.PREANALYZE_CASES[case]
    buf, org, stride = bc.preanalyze_plane(content, w, h, bd)
    ctx = capi.Context(w, h, bd)
    act, avg = ctx.preanalyze(buf, org, stride, depth)
    off = ctx.aq_layout(depth)
    for d in range(depth):
        ea = np.zeros(off[d + 1] - off[d])
        ev = oracle.fho_preanalyze_layer(op.ptr(buf.reshape(-1), org), stride, w, h, 64 >> d, ea)
        assert act[off[d]:off[d + 1]].tobytes() == ea.tobytes() and avg[d] == ev, (content, bd, d)
    dev = torch_cuda.device("cuda:0")
    d16 = torch_cuda.from_numpy(np.stack([buf, buf[::-1].copy()])).to(dev)
    dact = torch_cuda.zeros((2, off[-1]), dtype=torch_cuda.float64, device=dev)
    torch_cuda.cuda.synchronize()
    ctx.preanalyze_frames_device(d16.data_ptr() + 2 * org, 2, stride, buf.size, 2, dact.data_ptr(), max_aq_depth=depth)
    torch_cuda.cuda.synchronize()
    assert dact[0].cpu().numpy().tobytes() == act.tobytes()
    ctx.close()


@pytest.mark.parametrize("bd", [9, 11])
def test_host_batch_int16_planes(oracle, bd):
    w = weights.random_weights(5)
    planes = [_native(bd, seed=s) for s in (4, 5)]
    buf = np.stack([p[0] for p in planes])
    org, stride = planes[0][1], planes[0][2]
    ctx = capi.Context(W, H, bd, w, max_frames=2)
    d, h = ctx.predict_frames(buf, qp=32, origin=org, stride=stride, frame_stride=buf[0].size)
    for f in range(2):
        ed, _, eh = _oracle_predict(oracle, w, buf[f], org, stride, bd, 32)
        assert np.array_equal(d[f], ed) and np.array_equal(h[f], eh), f
    ctx.close()


# ---- blobs at the requant limits ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blob", ["conv2-edge", "conv2-over", "conv3-edge", "conv3-over", "conv3-high"])
def test_base_blobs_at_the_requant_limit(oracle, torch_cuda, blob, cnn_arith):
    layer, side = blob.split("-")
    w = weights.requant_limit_weights("high" if side == "high" else int(layer[-1]), over=side == "over")
    buf, org, stride = _native(10, seed=6)
    exp_d, exp_l, _ = _oracle_predict(oracle, w, buf, org, stride, 10, 32)
    ctx = capi.Context(W, H, 10, w)
    d, _ = ctx.predict_frame(buf, org, stride, qp=32)
    assert np.array_equal(d, exp_d)
    dd, lg, fl = _device_logits(torch_cuda, ctx, buf, org, stride, 32)
    assert np.array_equal(lg, exp_l) and np.array_equal(dd, exp_d)
    _check_flags(oracle, lg, fl)
    ctx.close()


@pytest.mark.parametrize("over", [False, True])
@pytest.mark.parametrize("requant", ["default", "general"])
def test_family_blob_at_the_requant_limit(oracle, torch_cuda, monkeypatch, over, requant):
    if requant == "general":
        monkeypatch.setenv("FHEVC_D2_REQUANT", "general")
    else:
        monkeypatch.delenv("FHEVC_D2_REQUANT", raising=False)
    f = weights.requant_limit_family(over=over)
    buf, org, stride = _native(10, seed=7)
    exp_d, exp_l, _ = _oracle_predict(oracle, f, buf, org, stride, 10, 32)
    ctx = capi.Context(W, H, 10, f)
    d, _ = ctx.predict_frame(buf, org, stride, qp=32)
    assert np.array_equal(d, exp_d)
    dd, lg, fl = _device_logits(torch_cuda, ctx, buf, org, stride, 32)
    assert np.array_equal(lg, exp_l) and np.array_equal(dd, exp_d)
    ctx.close()
