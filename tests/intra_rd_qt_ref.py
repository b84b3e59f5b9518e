"""Expected values of the RD estimate of the intra candidate with the depth count as an argument (fhevc_intra_rd_qt*, fhevc_p_tree_rd_intra_qt_frame),
restated in numpy from the definition in include/fasthevc.h -- not from the C code.  The prediction is intra_rd_ref's composition of the oracle's four intra
functions, extended to n = 4; per TU the arithmetic is motion_rd_ref's (pinned to the reference's own transforms and quantiser), with HM's DST-VII at the
intra 4x4 TUs (pinned to the reference's xTrMxN / xITrMxN with useDST by tests/golden/ref_dst.npz); the nested choice is a pure function of per-TU (D, r)
arrays, of which two depths are the `third=False` case; gate and fold are intra_rd_ref's.  tests/test_intra_rd_qt_ref.py holds this module against
intra_rd_ref and against closed forms without a GPU; tests/test_gpu_intra_rd_qt.py compares the library with it.  A plain module, not a conftest and not
a test."""
import functools

import numpy as np

import intra_rd_ref as ir
import motion_rd_ref as rd
import motion_refine_ref as mr

MARK, SAT = rd.MARK, rd.SAT
PDT = ir.PDT
TU_SIZES = {2: {64: (32, 16), 32: (32, 16), 16: (16, 8), 8: (8,)}, 3: {64: (32, 16), 32: (32, 16, 8), 16: (16, 8, 4), 8: (8, 4)}}   # node side -> TU size per depth
DST = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)   # g_as_DST_MAT_4 (TComRom.cpp:513-517)
LO, HI = -32768, 32767


def dst_forward(blocks, bd):
    """xTrMxN with useDST of [..., 4, 4] residuals: fastForwardDst twice, the shifts of the 4-point DCT -> [..., vertical frequency, horizontal frequency]"""
    blocks = np.asarray(blocks, np.int64)
    assert blocks.shape[-2:] == (4, 4)
    s1, s2 = rd.sk.shifts(4, bd)
    tmp = (blocks @ DST.T + (1 << (s1 - 1))) >> s1
    return (DST @ tmp + (1 << (s2 - 1))) >> s2


def dst_inverse(coef, bd):
    """xITrMxN with useDST of [..., 4, 4] coefficients: fastInverseDst twice, shift 7 then 20 - bd, both clipped to 16 bits -> the residual [..., y, x]"""
    coef = np.asarray(coef, np.int64)
    assert coef.shape[-2:] == (4, 4)
    s2 = 20 - bd
    tmp = np.clip((np.swapaxes(coef, -1, -2) @ DST + 64) >> 7, LO, HI)
    return np.clip((np.swapaxes(tmp, -1, -2) @ DST + (1 << (s2 - 1))) >> s2, LO, HI)


def tu_pass(org, pred, bd, qp, dst=True):
    """motion_rd_ref.tu_pass for intra TUs: [..., n, n] -> D, r, cbf, zero_half; a 4x4 TU goes through the DST (dst=False: the DCT, for comparisons)"""
    n = org.shape[-1]
    if n != 4 or not dst:
        return rd.tu_pass(org, pred, bd, qp)
    coef = dst_forward(np.asarray(org, np.int64) - pred, bd)
    lv = rd.levels(coef, 4, bd, qp)
    d, clipped = rd.sse(org, pred, dst_inverse(rd.dequant(lv, 4, bd, qp), bd), bd)
    return dict(D=d, r=rd.tu_bits(lv), cbf=(lv != 0).any(axis=(-1, -2)), zero_half=~(rd.levels(coef, 4, bd, qp, half=True) != 0).any(axis=(-1, -2)), clipped=clipped,
                levels=lv)


def nested_choice(D0, r0, D1, r1, D2, r2, lam, third=True, depth1=True):
    """one depth-0 TU: D0, r0 [...]; its four depth-1 TUs [..., 4]; their four children each [..., 4, 4] (ignored unless `third`).  HM's intra rule:
    dSplitCost < dSingleCost alone, strictly, at both depths.  depth1=False: a TU with no depth 1 (an 8x8 node at two depths) -> dict of J (the chosen cost
    without side bits), dist, rate (everything lam multiplies in J), take0 [...], take1 [..., 4] (masked by take0), would1 (unmasked), K1, K2, J0, J1"""
    D0, r0, D1, r1 = (np.asarray(a, np.int64) for a in (D0, r0, D1, r1))
    if third:
        D2s, r2s = np.asarray(D2, np.int64).sum(axis=-1), np.asarray(r2, np.int64).sum(axis=-1)
        K1 = 256 * D1 + lam * (1 + r1)                    # with this TU's own split flag
        K2 = 256 * D2s + lam * (1 + r2s)
        take1 = K2 < K1
    else:
        D2s, r2s = np.zeros_like(D1), np.zeros_like(r1)
        K1 = 256 * D1 + lam * r1                          # no flag: it cannot split
        K2 = np.zeros_like(K1)
        take1 = np.zeros(K1.shape, bool)
    C = np.where(take1, K2, K1)
    J0 = 256 * D0 + lam * (1 + r0)
    J1 = C.sum(axis=-1) + lam
    take0 = (J1 < J0) if depth1 else np.zeros(J0.shape, bool)
    own = (1 if third else 0) + np.where(take1, r2s, r1)   # what lam multiplies in C
    return dict(J=np.where(take0, J1, J0), dist=np.where(take0, np.where(take1, D2s, D1).sum(axis=-1), D0), rate=np.where(take0, 1 + own.sum(axis=-1), 1 + r0),
                take0=take0, take1=take1 & take0[..., None], would1=take1, K1=K1, K2=K2, J0=J0, J1=J1)


def node_from_choice(ch, cbf0, zero_half, side, lam):
    """ch: nested_choice over [M, T] depth-0 TUs -> (dist, cost_rd, bits, flags, tu_split) [M]"""
    side = np.asarray(side, np.int64)
    T = ch["take0"].shape[-1]
    j = ch["J"].sum(axis=-1) + lam * side
    bits = ch["rate"].sum(axis=-1) + side
    flags = np.where(~cbf0.any(axis=-1), rd.ZERO_PLAIN, 0) | np.where(zero_half.all(axis=-1), rd.ZERO_HALF, 0) | np.where(ch["take0"].any(axis=-1), rd.TU_SPLIT, 0)
    tu_split = (ch["take0"].astype(np.int64) << np.arange(T)).sum(axis=-1)
    if T == 1:
        tu_split = tu_split | (ch["take1"][:, 0].astype(np.int64) << (4 + np.arange(4))).sum(axis=-1)   # zero unless bit 0 is set: take1 is masked by take0
    return ch["dist"].sum(axis=-1), np.minimum(j >> 8, SAT), np.minimum(bits, 65535), flags, tu_split


def node_records(org, preds, bd, qp, side, detail=None, dst=True):
    """org [M, s, s]; preds: one [M, s, s] prediction per TU depth of the node (1 to 3 of them: an intra TU is predicted from its own neighbours, so the
    depths differ), side [M] -> (dist, cost_rd, bits, flags, tu_split) arrays [M]"""
    s = org.shape[-1]
    n0 = min(s, 32)
    lam = rd.lam_q8(qp)
    o0 = rd.split(np.asarray(org, np.int64), n0)                                             # [M, T, n0, n0]
    a = tu_pass(o0, rd.split(np.asarray(preds[0], np.int64), n0), bd, qp, dst)
    zero = np.zeros(a["D"].shape + (4,), np.int64)
    b = dict(D=zero, r=zero)
    c = dict(D=None, r=None, cbf=None)
    if len(preds) >= 2:
        o1 = rd.split(o0, n0 // 2)                                                           # [M, T, 4, n1, n1]
        b = tu_pass(o1, rd.split(rd.split(np.asarray(preds[1], np.int64), n0), n0 // 2), bd, qp, dst)
    if len(preds) == 3:
        c = tu_pass(rd.split(o1, n0 // 4), rd.split(rd.split(rd.split(np.asarray(preds[2], np.int64), n0), n0 // 2), n0 // 4), bd, qp, dst)   # [M, T, 4, 4, n2, n2]
    ch = nested_choice(a["D"], a["r"], b["D"], b["r"], c["D"], c["r"], lam, len(preds) == 3, len(preds) >= 2)
    if detail is not None:
        detail.update(ch, depths=len(preds), cbf2=c["cbf"])
        if len(preds) == 3:
            detail["two"] = nested_choice(a["D"], a["r"], b["D"], b["r"], None, None, lam, False)   # the same node at two depths
    return node_from_choice(ch, a["cbf"], a["zero_half"], side, lam)


def node_preds(P, x0, y0, s, mode, tu_depths):
    """the node's prediction assembled from its TUs, per depth -> a list of [s, s]"""
    out = []
    for n in TU_SIZES[tu_depths][s]:
        p = np.zeros((s, s), np.int64)
        for ty in range(0, s, n):
            for tx in range(0, s, n):
                p[ty:ty + n, tx:tx + n] = P.predict(x0 + tx, y0 + ty, n, mode)
        out.append(p)
    return out


def plain(pic, bd, qp, first, tu_depths=3, rows=None, details=None, dst=True):
    """pic [H, W] (or an intra_rd_ref.Picture), first [band CTUs, 85] NODE_DTYPE (any bytes) -> the plain intra RD records [band CTUs, 85]; details: a dict
    that takes, per level, the nested choice's arrays"""
    assert tu_depths in (2, 3)
    P = pic if isinstance(pic, ir.Picture) else ir.Picture(pic, bd)
    W, H = P.W, P.H
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    first = first.reshape(nb, 85)
    out = np.zeros((nb, 85), PDT)
    out[:] = ir.MARKER
    todo = {l: [] for l in range(4)}
    for i in range(nb):
        c = rows[0] * cw + i
        cx, cy = c % cw, c // cw
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            s = 64 >> lvl
            x0, y0 = cx * 64 + bx * s, cy * 64 + by * s
            mode = int(first[i, k]["mode"]) & 0xFF
            if x0 + s > W or y0 + s > H or int(first[i, k]["satd"]) == MARK or mode > 34:
                continue
            todo[lvl].append((i, k, P.pic[y0:y0 + s, x0:x0 + s], node_preds(P, x0, y0, s, mode, tu_depths), mode))
    for lvl, items in todo.items():
        if not items:
            continue
        detail = {} if details is not None else None
        preds = [np.stack([t[3][d] for t in items]) for d in range(len(items[0][3]))]
        dist, cost, bits, flags, tus = node_records(np.stack([t[2] for t in items]), preds, bd, qp, [ir.mode_bits(t[4]) for t in items], detail, dst)
        for m, (i, k, _, _, mode) in enumerate(items):
            out[i, k] = (int(dist[m]), int(cost[m]), int(bits[m]), int(flags[m]), int(tus[m]), ir.PART_INTRA, 0, (mode, 0))
        if details is not None:
            detail["where"] = [(t[0], t[1]) for t in items]
            details[lvl] = detail
    return out


def expected(pic, bd, qp, first, tu_depths=3, fold=None, rd_merge=None, skip_mask=0, rows=None, details=None, outcome=None):
    """one picture -> [band CTUs, 85] MOTION_RD_PU_DTYPE; fold / rd_merge compact over the same rows, or None"""
    p = plain(pic, bd, qp, first, tu_depths, rows, details)
    return ir.gate_fold(p, None if fold is None else fold.reshape(p.shape), None if rd_merge is None else rd_merge.reshape(p.shape), skip_mask, outcome)


same = ir.same


@functools.lru_cache(maxsize=None)
def draw(index, tu_depths=3):
    """entry `index` of intra_rd_ref's DRAW at tu_depths -> dict: bd, qp, pic, first, plain, details, fold, merge.  fold and merge are intra_rd_ref's records,
    drawn around the TWO-depth costs: both folds see the same inter records, as a caller's would"""
    d = ir.draw(index)
    details = {}
    p = plain(d["pic"], d["bd"], d["qp"], d["first"], tu_depths, details=details)
    return dict(bd=d["bd"], qp=d["qp"], pic=d["pic"], first=d["first"], plain=p, details=details, fold=d["fold"], merge=d["merge"])


# ---- closed-form pictures ------------------------------------------------------------------------------------------------------------------------------------

def constant_picture(W, H, bd, value=None):
    return np.full((H, W), (1 << (bd - 1)) + 3 if value is None else value, np.int64)


def stripes(W, H, bd, vertical, seed=3):
    """columns (vertical) or rows of random values: mode 26 (10) predicts every TU of every size exactly wherever the line above (left) is available"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << bd, size=W if vertical else H)
    return np.tile(v, (H, 1)) if vertical else np.tile(v[:, None], (1, W))


def bumped(W, H, bd, x0, y0, amp=40):
    """a constant picture with a checkerboard of +-amp confined to the 4x4 block at (x0, y0)"""
    pic = constant_picture(W, H, bd)
    yy, xx = np.mgrid[0:4, 0:4]
    pic[y0:y0 + 4, x0:x0 + 4] += np.where((xx + yy) % 2 == 0, amp, -amp)
    return pic
