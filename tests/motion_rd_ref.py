"""Expected values of the RD stage (fhevc_motion_rd*) and of the tree that takes its costs (fhevc_p_tree_select_rd*), restated in numpy from the
definitions in include/fasthevc.h -- not from the C code -- and laid over motion_skip_ref (the matrices, the quantiser's numbers, the tree rule) and
motion_refine_ref (the prediction): HM's forward transform xTrMxN now also at N = 4, the plain quantiser, xDeQuant without scaling lists, xITrMxN with
its two clips, xGetSSE with its per-sample shift, the library's own bit estimate, and the choice between one TU and its four children per depth-0 TU.
Everything is batched over leading axes and exact in int64.  tests/test_motion_rd_ref.py pins this module to the reference's own transforms
(tests/golden/ref_transform.npz, ref_inverse_transform.npz) and quantiser (ref_quant.npz) without a GPU; tests/test_motion_rd_abi.py and
tests/test_gpu_motion_rd.py compare the library with it.  A plain module, not a conftest and not a test."""
import math

import numpy as np

import motion_refine_ref as mr
import motion_skip_ref as sk
from fasthevc_amd import capi

MARK = 0xFFFFFFFF
SAT = 0xFFFFFFFE
RDT = capi.MOTION_RD_DTYPE
MERGE, EXPLICIT = capi.RD_SOURCE_MERGE, capi.RD_SOURCE_EXPLICIT
ZERO_PLAIN, ZERO_HALF, TU_SPLIT = 1, 2, 4
INVALID = (MARK, MARK, 0xFFFF, 0, 0, 0, 0)
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)                  # g_invQuantScales
LO, HI = -32768, 32767
TU_SIZES = {64: (32, 16), 32: (32, 16), 16: (16, 8), 8: (8, 4)}   # node side -> the depth-0 and the depth-1 TU size

log2 = sk.log2


def matrix(n):
    """the n-point DCT matrix [k][x], n = 4, 8, 16, 32: rows 0, 32 / n, .. of the 32-point one, its first n columns"""
    return sk.matrix(n)


def forward(blocks, bd, stages=False):
    """xTrMxN of [..., n, n] residuals (the DCT, maxLog2TrDynamicRange 15) -> coefficients [..., vertical frequency, horizontal frequency], int64"""
    blocks = np.asarray(blocks, np.int64)
    n = blocks.shape[-1]
    m, (s1, s2) = matrix(n), sk.shifts(n, bd)
    tmp = (blocks @ m.T + (1 << (s1 - 1))) >> s1               # partialButterfly over the rows: [..., row, horizontal frequency]
    out = (m @ tmp + (1 << (s2 - 1))) >> s2                    # ... over the columns
    return (tmp, out) if stages else out


def inverse(coef, bd, stages=False):
    """xITrMxN of [..., n, n] coefficients [vertical frequency, horizontal frequency] -> the residual [..., y, x]: the first stage over the vertical
    frequencies with shift 7, the second with shift 20 - bd, both clipped to 16 bits"""
    coef = np.asarray(coef, np.int64)
    m = matrix(coef.shape[-1])
    s2 = 20 - bd
    tmp = np.clip((np.swapaxes(coef, -1, -2) @ m + 64) >> 7, LO, HI)              # [..., horizontal frequency j, y] = sum_k m[k][y] coef[k][j]
    out = np.clip((np.swapaxes(tmp, -1, -2) @ m + (1 << (s2 - 1))) >> s2, LO, HI)   # [..., y, x] = sum_j m[j][x] tmp[j][y]
    return (tmp, out) if stages else out


def levels(coef, n, bd, qp, half=False):
    """the signed levels of the plain quantiser (half: under add_half), clipped to int16"""
    scale, qbits, add_plain, add_half = sk.quant(n, bd, qp)
    coef = np.asarray(coef, np.int64)
    mag = (np.abs(coef) * scale + (add_half if half else add_plain)) >> qbits
    return np.clip(np.sign(coef) * mag, LO, HI)


def right_shift(n, bd, qp):
    """xDeQuant's rightShift from HM's own expression: IQUANT_SHIFT - (transform shift + per)"""
    per = (qp + 6 * (bd - 8)) // 6
    return 6 - ((15 - bd - log2(n)) + per)


def target_input_bit_depth(n, bd, qp):
    """min(maxLog2TrDynamicRange + 1, 8 sizeof(Intermediate_Int) + rightShift - scaleBits), scaleBits = IQUANT_SHIFT + 1"""
    return min(16, 32 + right_shift(n, bd, qp) - 7)


def dequant(lv, n, bd, qp):
    """xDeQuant without scaling lists (TComTrQuant.cpp:1387-1422)"""
    rs, scale = right_shift(n, bd, qp), INV_QUANT_SCALES[(qp + 6 * (bd - 8)) % 6]
    t = target_input_bit_depth(n, bd, qp)
    q = np.clip(np.asarray(lv, np.int64), -(1 << (t - 1)), (1 << (t - 1)) - 1)
    c = (q * scale + (1 << (rs - 1))) >> rs if rs > 0 else (q * scale) << -rs
    return np.clip(c, LO, HI)


def tu_bits(lv):
    """r(TU) over the last two axes: 1 + sum over the non-zero levels of 3 + 2 floor(log2 |level|)"""
    a = np.abs(np.asarray(lv, np.int64))
    fl = np.zeros_like(a)
    for b in range(1, 16):
        fl += (a >> b) != 0                                    # floor(log2 a) of a >= 1
    return 1 + np.where(a != 0, 3 + 2 * fl, 0).sum(axis=(-1, -2))


def sse(org, pred, rhat, bd):
    """xGetSSE with its per-sample shift, over the last two axes -> (D, the number of rebuilt samples that were clipped)"""
    top = (1 << bd) - 1
    raw = np.asarray(pred, np.int64) + rhat
    e = np.asarray(org, np.int64) - np.clip(raw, 0, top)
    return ((e * e) >> (2 * (bd - 8))).sum(axis=(-1, -2)), ((raw < 0) | (raw > top)).sum(axis=(-1, -2))


def lam_q8(qp):
    return int(math.floor(0.57 * 2.0 ** ((qp - 12) / 3.0) * 256.0 + 0.5))


def split(a, n):
    """[..., S, S] -> [..., (S / n)^2, n, n], the blocks in raster order"""
    s = a.shape[-1]
    lead = a.shape[:-2]
    return a.reshape(lead + (s // n, n, s // n, n)).swapaxes(-3, -2).reshape(lead + ((s // n) ** 2, n, n))


def tu_pass(org, pred, bd, qp):
    """[..., n, n] TUs -> dict of per-TU arrays: D, r, cbf, zero_half, clipped, and the levels"""
    n = org.shape[-1]
    coef = forward(np.asarray(org, np.int64) - pred, bd)
    lv = levels(coef, n, bd, qp)
    d, clipped = sse(org, pred, inverse(dequant(lv, n, bd, qp), bd), bd)
    return dict(D=d, r=tu_bits(lv), cbf=(lv != 0).any(axis=(-1, -2)), zero_half=~(levels(coef, n, bd, qp, half=True) != 0).any(axis=(-1, -2)), clipped=clipped,
                levels=lv)


def tu_choice(d0, r0, d1, r1, any1, lam):
    """one depth-0 TU against its four children (d1, r1: their sums) -> (J0, J1, split taken); strict, as TEncSearch.cpp:5117"""
    j0 = 256 * np.asarray(d0, np.int64) + lam * (1 + np.asarray(r0, np.int64))
    j1 = 256 * np.asarray(d1, np.int64) + lam * (1 + np.asarray(r1, np.int64))
    return j0, j1, np.asarray(any1, bool) & (j1 < j0)


def node_records(org, pred, bd, qp, side, detail=None):
    """org, pred: [M, s, s] nodes of one size, side: [M] side bits -> (dist, cost_rd, bits, flags, tu_split) arrays [M]; detail: a dict that takes the
    per-TU numbers"""
    s = org.shape[-1]
    n0, n1 = TU_SIZES[s]
    lam = lam_q8(qp)
    o0, p0 = split(np.asarray(org, np.int64), n0), split(np.asarray(pred, np.int64), n0)       # [M, T, n0, n0]
    a = tu_pass(o0, p0, bd, qp)
    b = tu_pass(split(o0, n1), split(p0, n1), bd, qp)                                          # [M, T, 4, n1, n1]
    d1, r1, any1 = b["D"].sum(axis=-1), b["r"].sum(axis=-1), b["cbf"].any(axis=-1)
    j0, j1, take = tu_choice(a["D"], a["r"], d1, r1, any1, lam)
    side = np.asarray(side, np.int64)
    j = np.where(take, j1, j0).sum(axis=-1) + lam * side
    dist = np.where(take, d1, a["D"]).sum(axis=-1)
    bits = (1 + np.where(take, r1, a["r"])).sum(axis=-1) + side
    flags = np.where(~a["cbf"].any(axis=-1), ZERO_PLAIN, 0) | np.where(a["zero_half"].all(axis=-1), ZERO_HALF, 0) | np.where(take.any(axis=-1), TU_SPLIT, 0)
    tu_split = (take.astype(np.int64) << np.arange(take.shape[-1])).sum(axis=-1)
    if detail is not None:
        detail.update(J0=j0, J1=j1, take=take, cbf0=a["cbf"], any1=any1, D0=a["D"], r0=a["r"], D1=d1, r1=r1, clipped=a["clipped"] + b["clipped"].sum(axis=-1),
                      levels0=a["levels"], levels1=b["levels"])
    return dist, np.minimum(j >> 8, SAT), np.minimum(bits, 65535), flags, tu_split


def merge_side_bits(idx):
    idx = np.asarray(idx, np.int64)
    return np.where(idx == 4, 4, idx + 1)


def explicit_side_bits(mvx, mvy):
    return np.array([mr.eg_bits(int(x)) + mr.eg_bits(int(y)) for x, y in zip(np.ravel(mvx), np.ravel(mvy))], np.int64).reshape(np.shape(mvx))


class Stats:
    """what a draw exercised, per level 0..3: depth-0 TUs with the split taken / not taken, with cbf 0 / != 0, and with a clipped rebuilt sample"""

    def __init__(self):
        self.n = {k: [0, 0, 0, 0] for k in ("taken", "not_taken", "cbf0", "cbf1", "clipped")}

    def add(self, lvl, detail):
        t, c = detail["take"], detail["cbf0"]
        for k, v in (("taken", t.sum()), ("not_taken", (~t).sum()), ("cbf0", (~c).sum()), ("cbf1", c.sum()), ("clipped", (detail["clipped"] > 0).sum())):
            self.n[k][lvl] += int(v)


def expected(cur, ref_pic, W, H, bd, qp, records, source, max_range, mvp=None, rows=None, planes=None, stats=None):
    """cur / ref_pic: the samples [H, W]; records: [band CTUs, 85] MOTION_MERGE_DTYPE (source MERGE) or MOTION_QPEL_DTYPE (EXPLICIT), mvp: as many
    MOTION_MVP_DTYPE or None; all compact over the CTU rows `rows` -> [band CTUs, 85] MOTION_RD_DTYPE"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    records = records.reshape(nb, 85)
    assert source in (MERGE, EXPLICIT) and (mvp is None or source == EXPLICIT)
    mvp = mvp.reshape(nb, 85) if mvp is not None else None
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    assert planes.pad >= max_range + 6 and planes.bd == bd
    cur = np.asarray(cur, np.int64)
    reach = 4 * max_range + 3
    out = np.zeros((nb, 85), RDT)
    out[:] = INVALID
    todo = {l: [] for l in range(4)}
    for i in range(nb):
        c = rows[0] * cw + i
        cx, cy = c % cw, c // cw
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            n = 64 >> lvl
            x0, y0 = cx * 64 + bx * n, cy * 64 + by * n
            rec = records[i, k]
            q = (int(rec["mvx"]), int(rec["mvy"]))
            if x0 + n > W or y0 + n > H or int(rec["cost_best"]) == MARK or abs(q[0]) > reach or abs(q[1]) > reach:
                continue
            if source == MERGE:
                side = int(merge_side_bits(rec["idx"]))
            elif mvp is not None:
                if int(mvp[i, k]["idx"]) == 255:
                    continue
                side = int(mvp[i, k]["bits"])
            else:
                side = mr.eg_bits(q[0]) + mr.eg_bits(q[1])
            todo[lvl].append((i, k, cur[y0:y0 + n, x0:x0 + n], planes.block(q[0], q[1], x0, y0, n).astype(np.int64), side, q))
    for lvl, items in todo.items():
        if not items:
            continue
        detail = {} if stats is not None else None
        dist, cost, bits, flags, tus = node_records(np.stack([t[2] for t in items]), np.stack([t[3] for t in items]), bd, qp, [t[4] for t in items], detail)
        for m, (i, k, _, _, _, q) in enumerate(items):
            out[i, k] = (int(dist[m]), int(cost[m]), int(bits[m]), int(flags[m]), int(tus[m]), q[0], q[1])
        if stats is not None:
            stats.add(lvl, detail)
    return out


def same(got, exp, what=""):
    """every byte of every record"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    for f in RDT.names:
        bad = got[f] != exp[f]
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())


# ---- the tree on RD records: the skip tree with three substitutions --------------------------------------------------------------------------------------

def tree_select(rd_explicit, rd_merge, skip_mask, W, H, rows=None, rule=None):
    """rd_explicit / rd_merge: [P, band CTUs, 85] MOTION_RD_DTYPE -> (records, depth_min, depth_max) as motion_skip_ref.tree_select on cost_rd, cost_rd, flags"""
    sc, mc, sf = rd_explicit["cost_rd"], rd_merge["cost_rd"], rd_merge["flags"]
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rb, re = rows if rows is not None else (0, ch)
    P, nb = sc.shape[:2]
    assert nb == (re - rb) * cw
    rec, dmin, dmax = np.zeros((P, nb, 85), sk.pt.TDT), np.zeros((P, nb, 256), np.uint8), np.zeros((P, nb, 256), np.uint8)
    for p in range(P):
        for i in range(nb):
            rec[p, i], dmin[p, i], dmax[p, i] = sk.tree_ctu(sc[p, i], mc[p, i], sf[p, i], skip_mask, *sk.pt.valid_size(rb * cw + i, W, H), rule)
    return rec, dmin, dmax


# ---- the draw: a 168 x 152 picture pair -- two whole CTUs in either direction, ragged in both -- and records of both kinds ---------------------------------

DRAW_W, DRAW_H = 168, 152
DRAW_CW, DRAW_CH = 3, 3
DRAW_N = DRAW_CW * DRAW_CH
DRAW_QPS = (4, 10, 14, 22, 27, 37, 51)


def draw_pictures(bd, seed=0):
    """reference and current picture [H, W] int64 at bd bits with the low bits in use: smooth structure that pans by a fraction, texture of mixed strength,
    a near-binary strip (rebuilt samples clip there) and a flat corner under faint noise (cbf 0 at all but the lowest QPs)"""
    rng = np.random.default_rng(1000 + 16 * seed + bd)
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:DRAW_H + 8, 0:DRAW_W + 8].astype(np.float64)
    base = 0.5 + 0.22 * np.sin(xx / 9.0) * np.cos(yy / 13.0) + 0.15 * np.sin((xx + 2 * yy) / 5.0)
    grain = rng.normal(0.0, 1.0, size=base.shape) * np.where((xx // 32 + yy // 32) % 2 == 0, 0.12, 0.015)
    big = np.clip((base + grain) * top, 0, top)
    strip = np.where(big[:, :40] > top / 2, top, 0)
    big[:, :40] = np.where(rng.random(strip.shape) < 0.92, strip, top - strip)                                        # a near-binary strip: rebuilt samples overshoot
    big[60:, 60:] = top // 3                                                                                          # a flat corner that holds one whole CTU
    ref = np.rint(big[4:4 + DRAW_H, 4:4 + DRAW_W]).astype(np.int64)
    moved = 0.5 * (big[3:3 + DRAW_H, 2:2 + DRAW_W] + big[3:3 + DRAW_H, 3:3 + DRAW_W])                                 # a pan by (1.5, 1) samples
    cur = np.clip(np.rint(moved + rng.normal(0.0, 0.004 * top, size=moved.shape)), 0, top).astype(np.int64)
    cur[70:110, 8:48] = np.clip(cur[70:110, 8:48] + rng.integers(-top // 3, top // 3, size=(40, 40)), 0, top)         # content the reference lacks
    return ref, cur


def draw_records(source, seed, max_range, shape=(DRAW_N, 85), with_mvp=False):
    """records of random bytes whose vectors lie near the pan, anywhere in the reach, on its limit or (one in ten) beyond it, one in seven marked ->
    (records, mvp or None)"""
    rng = np.random.default_rng(seed)
    dt = capi.MOTION_MERGE_DTYPE if source == MERGE else capi.MOTION_QPEL_DTYPE
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), dt).reshape(shape).copy()
    reach = 4 * max_range + 3
    kind = rng.random(shape)
    near = np.stack([np.clip(6 + rng.integers(-3, 4, size=shape), -reach, reach), np.clip(4 + rng.integers(-3, 4, size=shape), -reach, reach)], -1)
    anywhere = rng.integers(-reach, reach + 1, size=shape + (2,))
    edge = rng.choice([-reach, reach], size=shape + (2,))
    beyond = np.where(rng.random(shape) < 0.5, reach + 1, rng.integers(reach + 1, 32768, size=shape)) * rng.choice([-1, 1], size=shape)
    v = np.where((kind < 0.6)[..., None], near, np.where((kind < 0.8)[..., None], anywhere, edge))
    far = kind >= 0.9
    a["mvx"] = np.where(far & (rng.random(shape) < 0.5), beyond, v[..., 0])
    a["mvy"] = np.where(far & (a["mvx"] == v[..., 0]), beyond, v[..., 1])
    a["cost_best"] = np.where(rng.random(shape) < 1 / 7, MARK, a["cost_best"] % 100000)
    if source == MERGE:
        a["idx"] = rng.integers(0, 5, size=shape)
    mvp = None
    if with_mvp:
        mvp = np.frombuffer(rng.bytes(int(np.prod(shape)) * 8), capi.MOTION_MVP_DTYPE).reshape(shape).copy()
        mvp["idx"] = np.where(rng.random(shape) < 0.1, 255, rng.integers(0, 2, size=shape))
        mvp["bits"] = rng.integers(2, 67, size=shape)
    return a, mvp
