"""The oracle's integer depth classifier against an independent float64 torch restatement of the same network
(parity for this part is "unpinned" w.r.t. the reference: it ships no inference code or weights)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import oracle_py as op
from fasthevc_amd import frames, weights


def torch_cnn(w, ctu):
    """ctu: int8 [64,64] centred.  Exact in float64: every intermediate is an integer < 2^53."""
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    x = t(ctu).reshape(1, 1, 64, 64)
    acts = []
    for wk, bk, sh, pool in ((w["w1"].reshape(16, 1, 3, 3), w["b1"], w["shift"][0], True),
                             (w["w2"], w["b2"], w["shift"][1], True), (w["w3"], w["b3"], w["shift"][2], False)):
        x = Fn.conv2d(x, t(wk), t(bk), padding=1)
        if pool:
            x = Fn.max_pool2d(x, 2)
        x = torch.clamp(torch.floor(x / float(1 << int(sh))), 0, 255)
        acts.append(x[0].permute(1, 2, 0).numpy().astype(np.uint8))
    a3 = x[0].permute(1, 2, 0)  # [16,16,64]
    logits = np.zeros((21, 2), np.int64)
    pooled = (4 * Fn.avg_pool2d(x, 2))[0].permute(1, 2, 0)  # 2x2 sum pool, [8,8,64]
    for cls in range(2):
        logits[0, cls] = int((pooled * t(w["wh64"][cls])).sum()) + int(w["bh64"][cls])
        for q in range(4):
            qy, qx = q >> 1, q & 1
            logits[1 + q, cls] = int((a3[qy * 8:qy * 8 + 8, qx * 8:qx * 8 + 8] * t(w["wh32"][cls])).sum()) + int(w["bh32"][cls])
        for b in range(16):
            by, bx = b >> 2, b & 3
            logits[5 + b, cls] = int((a3[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] * t(w["wh16"][cls])).sum()) + int(w["bh16"][cls])
    qp = 27
    logits[0, 1] += int(w["qp_bias"][0, qp])
    logits[1:5, 1] += int(w["qp_bias"][1, qp])
    logits[5:, 1] += int(w["qp_bias"][2, qp])
    return acts, logits


def test_oracle_cnn_matches_torch_float64(oracle):
    rng = np.random.default_rng(11)
    luma = frames.texture16_luma(416, 240)
    for seed, extreme in ((0, False), (1, False), (2, True)):
        w = weights.random_weights(seed, extreme=extreme)
        ws = op.weights_from_arrays(w)
        for trial in range(3):
            if trial == 0:
                ctu = (luma[64:128, 128:192].astype(np.int16) - 128).astype(np.int8)
            elif trial == 1:
                ctu = rng.integers(-128, 128, size=(64, 64)).astype(np.int8)
            else:
                ctu = rng.choice(np.array([-128, 127], np.int8), size=(64, 64))
            ctu = np.ascontiguousarray(ctu)
            a1 = np.zeros(32 * 32 * 16, np.uint8)
            a2 = np.zeros(16 * 16 * 32, np.uint8)
            a3 = np.zeros(16 * 16 * 64, np.uint8)
            logits = np.zeros(42, np.int32)
            oracle.fho_cnn_ctu_debug(ws, ctu.reshape(-1), 27, a1, a2, a3, logits)
            acts, ref_logits = torch_cnn(w, ctu)
            assert np.array_equal(a1.reshape(32, 32, 16), acts[0])
            assert np.array_equal(a2.reshape(16, 16, 32), acts[1])
            assert np.array_equal(a3.reshape(16, 16, 64), acts[2])
            assert np.array_equal(logits.reshape(21, 2).astype(np.int64), ref_logits)


def test_exactness_bound_for_fp32_accumulation():
    # HISTORY.md section 4: |bias| <= 2^22 and K*255*127 keep every conv accumulator below 2^24,
    # so fp32 accumulation of the bf16 products on the GPU is exact in any order
    assert 9 * 128 * 127 + weights.BIAS_LIMIT < 1 << 24
    assert 144 * 255 * 127 + weights.BIAS_LIMIT < 1 << 24
    assert 288 * 255 * 127 + weights.BIAS_LIMIT < 1 << 24


def test_depth_from_logits_rules(oracle):
    lg = np.zeros((21, 2), np.int32)
    d = np.zeros(256, np.uint8)
    oracle.fho_depth_from_logits(lg.reshape(-1), 64, 64, d)
    assert d.max() == 0  # ties -> no split (class 1 must win strictly)
    lg[0] = (0, 1)
    oracle.fho_depth_from_logits(lg.reshape(-1), 64, 64, d)
    assert set(d.tolist()) == {1}
    lg[1 + 3] = (0, 5)       # bottom-right 32x32 splits
    lg[5 + 15] = (-1, 0)     # its bottom-right 16x16 splits to 8x8
    oracle.fho_depth_from_logits(lg.reshape(-1), 64, 64, d)
    m = d.reshape(16, 16)
    assert (m[:8, :] == 1).all() and (m[8:, :8] == 1).all() and (m[8:12, 8:] == 2).all() and (m[12:, 12:] == 3).all()
    # picture edge: a 64x64 CTU of which only 32x48 is inside -> 64 and the crossing 32s are forced to split
    lg[:] = 0
    oracle.fho_depth_from_logits(lg.reshape(-1), 32, 48, d)
    m = d.reshape(16, 16)
    assert (m[:8, :8] == 1).all()             # top-left 32x32 inside: no forced split, logits say no
    assert (m[8:12, :8] == 2).all()           # bottom-left 32x32 crosses the bottom edge -> split to 16x16
    assert (m[12:, :] == 0).all() and (m[:, 8:] == 0).all()  # outside the picture


def test_depth_range_from_logits(oracle):
    """Soft decisions: margin 0 is the plain map; ranges nest as the margin grows; forced splits at the picture edge
    are in both maps; a huge margin frees every decision the picture edge does not force."""
    rng = np.random.default_rng(4)
    for t in range(300):
        lg = rng.integers(-60, 60, (21, 2)).astype(np.int32)
        vw, vh = [(64, 64), (32, 64), (64, 48), (16, 8), (40, 64)][t % 5]
        plain, a0, b0 = (np.zeros(256, np.uint8) for _ in range(3))
        oracle.fho_depth_from_logits(lg.reshape(-1), vw, vh, plain)
        oracle.fho_depth_range_from_logits(lg.reshape(-1), vw, vh, 0, 0, a0, b0)
        assert np.array_equal(a0, plain) and np.array_equal(b0, plain)
        prev_a, prev_b = a0, b0
        for m in (5, 25, 1000):
            a, b = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
            oracle.fho_depth_range_from_logits(lg.reshape(-1), vw, vh, m, m, a, b)
            assert np.all(a <= prev_a) and np.all(prev_b <= b)
            a1, b1 = np.zeros(256, np.uint8), np.zeros(256, np.uint8)  # the two margins act independently
            oracle.fho_depth_range_from_logits(lg.reshape(-1), vw, vh, m, 0, a1, b1)
            assert np.array_equal(a1, a) and np.array_equal(b1, plain)
            prev_a, prev_b = a, b
        forced = np.zeros(256, np.uint8)  # what the picture edge alone forces: all logits say "stop"
        oracle.fho_depth_from_logits(np.tile(np.array([1, 0], np.int32), 21), vw, vh, forced)
        assert np.array_equal(prev_a, forced)
        inside = np.zeros((16, 16), bool)
        inside[:vh // 4, :vw // 4] = True
        assert np.all(prev_b.reshape(16, 16)[inside] == 3) and np.all(prev_b.reshape(16, 16)[~inside] == 0)


def test_predict_frame_edge_ctus(oracle):
    w = weights.random_weights(5)
    ws = op.weights_from_arrays(w)
    luma = frames.texture16_luma(416, 240)
    buf, org, stride = frames.to_pel_plane(luma, 8)
    depth = np.zeros(28 * 256, np.uint8)
    oracle.fho_predict_frame(ws, op.ptr(buf.reshape(-1), org), stride, 416, 240, 8, 32, depth, None)
    depth = depth.reshape(4, 7, 16, 16)
    assert (depth[:, 6, :, 8:] == 0).all()     # last CTU column is 32 px wide
    assert (depth[3, :, 12:, :] == 0).all()    # last CTU row is 48 px tall
    assert (depth[3, :6, 8:12, :] >= 2).all()  # 32x32 blocks crossing the bottom edge are split
    assert (depth[:3, 6, :, :8] >= 1).all()    # CTUs crossing the right edge are split at 64


def test_split_flag_word_equals_depth_map(oracle):
    """The 21-bit word (what the ranks all-gather) carries exactly the depth map, picture edges included."""
    rng = np.random.default_rng(9)
    for _ in range(400):
        lg = rng.integers(-5, 6, size=(21, 2)).astype(np.int32)
        vw, vh = int(rng.choice([64, 64, 64, 56, 48, 32, 16, 8])), int(rng.choice([64, 64, 64, 56, 48, 40, 24, 8]))
        d_ref = np.zeros(256, np.uint8)
        oracle.fho_depth_from_logits(lg.reshape(-1), vw, vh, d_ref)
        word = oracle.fho_flags_from_logits(lg.reshape(-1), vw, vh)
        assert word < (1 << 21)
        d = np.zeros(256, np.uint8)
        oracle.fho_depth_from_flags(word, vw, vh, d)
        assert np.array_equal(d, d_ref), (vw, vh, hex(word))


def test_family_oracle_reproduces_the_base_network_and_a_float64_restatement(oracle):
    """The reference's Bayesian-optimisation family (fho_cnn_ctu_family; Optimize...Example.m:103-106, 233-259) in the oracle:
    (i) the depth-1 member with widths 16 / 32 / 64 IS the base network -- identical logits to fho_cnn_ctu on random CTUs;
    (ii) the depth-1 member 32 / 64 / 128 and the depth-2 member 23 / 46 / 92 against an independent float64 torch restatement."""
    import ctypes as C
    import torch
    import torch.nn.functional as Fn
    from oracle import oracle_py as op
    from fasthevc_amd import weights
    rng = np.random.default_rng(3)
    base = weights.random_weights(4)
    fam = op.family_from_arrays(weights.family_from_base(base))
    ws = op.weights_from_arrays(base)
    for _ in range(3):
        ctu = rng.integers(-128, 128, size=64 * 64).astype(np.int8)
        a, b = np.zeros(42, np.int32), np.zeros(42, np.int32)
        oracle.fho_cnn_ctu(ws, ctu, 27, a)
        oracle.fho_cnn_ctu_family(C.byref(fam), ctu.ctypes.data, 27, b.ctypes.data)
        assert np.array_equal(a, b)
    assert weights.family_widths(1) == (32, 64, 128) and weights.family_widths(2) == (23, 46, 92) and weights.family_widths(3) == (18, 36, 72)  # 2 * and 4 * the ROUNDED first width (:242, :248, :253)
    for depth in (1, 2):
        w = weights.random_family(weights.family_widths(depth), depth, seed=depth)
        assert weights.unpack_family(weights.pack_family(w))["w20"].shape == w["w20"].shape
        f = op.family_from_arrays(w)
        ctu = rng.integers(-128, 128, size=64 * 64).astype(np.int8)
        got = np.zeros(42, np.int32)
        oracle.fho_cnn_ctu_family(C.byref(f), ctu.ctypes.data, 32, got.ctypes.data)
        x = torch.from_numpy(ctu.astype(np.float64)).reshape(1, 1, 64, 64)
        for blk in range(3):
            for j in range(depth):
                z = Fn.conv2d(x, torch.from_numpy(w[f"w{blk}{j}"].astype(np.float64)), torch.from_numpy(w[f"b{blk}{j}"].astype(np.float64)), padding=1)
                if j == depth - 1 and blk < 2:
                    z = Fn.max_pool2d(z, 2)
                x = torch.clamp(torch.floor(z / float(1 << int(w["shift"][blk][j]))), 0, 255)
        a3 = x
        t = lambda k: torch.from_numpy(w[k].astype(np.float64)).permute(0, 3, 1, 2)
        l64 = Fn.conv2d(4.0 * Fn.avg_pool2d(a3, 2), t("wh64"), torch.from_numpy(w["bh64"].astype(np.float64))).flatten()
        l32 = Fn.conv2d(a3, t("wh32"), torch.from_numpy(w["bh32"].astype(np.float64)), stride=8)[0]
        l16 = Fn.conv2d(a3, t("wh16"), torch.from_numpy(w["bh16"].astype(np.float64)), stride=4)[0]
        exp = np.zeros((21, 2))
        exp[0] = l64.numpy()
        exp[1:5] = l32.reshape(2, 4).numpy().T
        exp[5:21] = l16.reshape(2, 16).numpy().T
        exp[0, 1] += w["qp_bias"][0, 32]; exp[1:5, 1] += w["qp_bias"][1, 32]; exp[5:, 1] += w["qp_bias"][2, 32]
        assert np.array_equal(got.reshape(21, 2), exp.astype(np.int64)), depth


def _bound(wl, b, first=False):
    """the library's requant bound (fhevc_weights.hip: folded_bias, for build_weight_image and the family loaders): max over outputs of |b'| + 128 sum |w|"""
    wl = np.asarray(wl, np.int64).reshape(len(b), -1)
    bp = np.asarray(b, np.int64) + (0 if first else 128 * wl.sum(1))
    return int((np.abs(bp) + 128 * np.abs(wl).sum(1)).max())


def _torch_accumulators(layers, ctu, wrap=None):
    """float64 restatement of a chain of conv3x3 layers [(w, b, shift, pool)]: -> (largest accumulator per layer, last map).
    wrap = layer index whose requant takes bytes 1-2 of the accumulator (the short form) instead of the general one."""
    t = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))
    x = t(ctu).reshape(1, 1, 64, 64)
    peaks = []
    for i, (wk, bk, sh, pool) in enumerate(layers):
        x = Fn.conv2d(x, t(wk), t(bk), padding=1)
        if pool:
            x = Fn.max_pool2d(x, 2)
        peaks.append(float(x.max()))
        if i == wrap:   # int16 of bits 8..23
            x = torch.remainder(torch.floor(x / 256) + 32768, 65536) - 32768
        else:
            x = torch.floor(x / float(1 << int(sh)))
        x = torch.clamp(x, 0, 255)
    return peaks, x


def _base_layers(w):
    return [(w["w1"].reshape(16, 1, 3, 3), w["b1"], w["shift"][0], True), (w["w2"], w["b2"], w["shift"][1], True), (w["w3"], w["b3"], w["shift"][2], False)]


def _family_layers(f):
    d = int(f["depth"])
    return [(f[f"w{b}{j}"], f[f"b{b}{j}"], f["shift"][b][j], j == d - 1 and b < 2) for b in range(3) for j in range(d)]


@pytest.mark.parametrize("layer", [2, 3])
def test_base_blobs_at_the_requant_limit(oracle, layer):
    """Bound of conv2 / conv3 at 2^23 - 1 (short form 2 chosen) and one past it (general form); flat content realises > 99 % of it:
    the edge blob's accumulator stays below 2^23, the over blob's reaches exactly 2^23, where the short form would give 0 instead of 255
    -- and that changes the logits, so a wrong form cannot hide behind a later clamp."""
    ctu = np.zeros((64, 64), np.int8)
    li = layer - 1
    for over in (False, True):
        w = weights.requant_limit_weights(layer, over)
        wl, bl = w[f"w{layer}"], w[f"b{layer}"]
        bound = _bound(wl, bl)
        assert int(w["shift"][li]) == 8 and (bound >= 1 << 23) == over
        assert bound == (1 << 23) - 1 + (0 if not over else int(np.asarray(wl).reshape(len(bl), -1).sum(1).max()) + 1)
        if layer == 3:  # conv2 keeps its short form 1 (shift 7): the conv3 bound alone decides between the kernel's short and general forms
            assert int(w["shift"][1]) == 7
        peaks, _ = _torch_accumulators(_base_layers(w), ctu)
        assert peaks[li] >= 0.99 * bound and (peaks[li] == 1 << 23) == over and peaks[li] <= bound
        acts, logits = torch_cnn(w, ctu)
        ws = op.weights_from_arrays(w)
        a1, a2, a3, lg = np.zeros(32 * 32 * 16, np.uint8), np.zeros(16 * 16 * 32, np.uint8), np.zeros(16 * 16 * 64, np.uint8), np.zeros(42, np.int32)
        oracle.fho_cnn_ctu_debug(ws, np.ascontiguousarray(ctu.reshape(-1)), 27, a1, a2, a3, lg)
        assert np.array_equal(lg.reshape(21, 2).astype(np.int64), logits)
        assert acts[li].max() == 255
        _, wrapped = _torch_accumulators(_base_layers(w), ctu, wrap=li)
        _, plain = _torch_accumulators(_base_layers(w), ctu)
        assert torch.equal(wrapped, plain) != over   # the short form is exact on the edge blob only
        if over:  # ... and the wrapped activations reach the logits
            a3w = wrapped[0].permute(1, 2, 0)
            assert not torch.equal(a3w, torch.from_numpy(acts[2].astype(np.float64)))
            assert int((a3w[:8, :8] * torch.from_numpy(w["wh32"][0].astype(np.float64))).sum()) + int(w["bh32"][0]) != logits[1, 0]


def test_high_conv3_accumulators_stay_exact_in_f16_and_take_the_general_form():
    w = weights.requant_limit_weights("high")
    assert _bound(w["w3"], w["b3"]) >= 1 << 23
    peaks, _ = _torch_accumulators(_base_layers(w), np.zeros((64, 64), np.int8))
    assert 13_000_000 < peaks[2] < 1 << 24


def test_family_blob_at_the_requant_limit(oracle):
    """The 23 / 46 / 92 x 2 member (k_cnn_d2.inc; d2_short when every bound is below 2^23) with every convolution after the first at
    the edge, and one past it."""
    import ctypes as C
    ctu = np.zeros((64, 64), np.int8)
    for over in (False, True):
        f = weights.requant_limit_family(over=over)
        layers = _family_layers(f)
        bounds = [_bound(wk, bk, first=(i == 0)) for i, (wk, bk, _, _) in enumerate(layers)]
        assert all((b >= 1 << 23) == over for b in bounds[1:]) and bounds[0] < 1 << 23
        peaks, _ = _torch_accumulators(layers, ctu)
        for i in range(1, len(layers)):
            assert peaks[i] >= 0.99 * bounds[i] and (peaks[i] == 1 << 23) == over, (i, peaks[i], bounds[i])
        # all-positive weights re-saturate behind a wrapped layer; the last one feeds the heads directly
        _, wrapped = _torch_accumulators(layers, ctu, wrap=len(layers) - 1)
        _, plain = _torch_accumulators(layers, ctu)
        assert torch.equal(wrapped, plain) != over
        # the oracle's family network is the same chain
        lg = np.zeros(42, np.int32)
        oracle.fho_cnn_ctu_family(C.byref(op.family_from_arrays(f)), C.c_void_p(np.ascontiguousarray(ctu).ctypes.data), 27, C.c_void_p(lg.ctypes.data))
        a3 = plain[0].permute(1, 2, 0)
        exp16 = int((a3[:4, :4] * torch.from_numpy(f["wh16"][0].astype(np.float64))).sum()) + int(f["bh16"][0])
        assert lg[2 * 5] == exp16
