"""Expected values of the zero-residual stage (fhevc_motion_skip*) and of the tree decision that takes its answer (fhevc_p_tree_select_skip*), restated
in Python from the definitions in include/fasthevc.h -- not from the C code: HM's forward DCT (xTrMxN) as two integer matrix products with its shifts and
rounding on int64 intermediates, the scalar quantiser without scaling lists in Python integers, expected() over a picture and a band on
motion_refine_ref's prediction, and the tree rule on p_tree_ref's geometry.  tests/test_motion_skip_ref.py pins this module to the reference's own
transform (tests/golden/ref_transform.npz) without a GPU, tests/test_motion_skip_quant_pin.py pins quant(), first_nonzero() and node_record() to the
reference's own quantiser, plain and RDOQ (tests/golden/ref_quant.npz), tests/test_motion_skip_abi.py compares the host functions with it,
tests/test_gpu_motion_skip.py the kernels.  All three readings of HM a record rests on are thereby pinned: the prediction (ref_frac_search*.npz through
motion_refine_ref.Planes), the transform, and the quantiser with its two zero bits.  A plain module, not a conftest and not a test."""
import numpy as np

import motion_merge_ref as mg
import motion_refine_ref as mr
import p_tree_ref as pt
from fasthevc_amd import capi

MARK = 0xFFFFFFFF
SDT = capi.MOTION_SKIP_DTYPE
ZERO_PLAIN, ZERO_HALF = 1, 2                                  # bits 0 and 1 of a skip record's flags
SKIPPED = 128                                                 # bit 7 of a tree record's flags
INVALID = (MARK, MARK, 0xFFFF, 0, 0, 0, 0)                    # the record of a node that is not valid
QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564)     # g_quantScales
# the 32 magnitudes of the standard's transform matrix (H.265 8.6.4.2): entry m is the scaled cos(m pi / 64), entry 0 the DC row's 64
_COS = (64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4)


_MATRICES = {}


def matrix(n):
    """the n-point DCT matrix, computed once"""
    if n not in _MATRICES:
        _MATRICES[n] = _matrix(n)
    return _MATRICES[n]


def _matrix(n):
    """the n-point DCT matrix [k][x] of the standard, n = 8, 16, 32: rows 0, 32 / n, 2 * 32 / n, .. of the 32-point one, its first n columns"""
    step = 32 // n
    m = np.zeros((n, n), np.int64)
    for k in range(n):
        for x in range(n):
            a = ((2 * x + 1) * k * step) % 128              # the angle in units of pi / 64
            a = 128 - a if a > 64 else a
            m[k, x] = -_COS[64 - a] if a > 32 else _COS[a]
    return m


def log2(n):
    return n.bit_length() - 1


def shifts(n, bd):
    return log2(n) + bd - 9, log2(n) + 6


def forward(block, bd, stages=False):
    """xTrMxN of an n x n block of residuals (DCT, maxLog2TrDynamicRange 15) -> coefficients [vertical frequency][horizontal frequency], int64;
    stages: (first-stage values [row][horizontal frequency], coefficients)"""
    block = np.asarray(block, np.int64)
    n = block.shape[0]
    assert block.shape == (n, n) and n in (8, 16, 32)
    m, (s1, s2) = matrix(n), shifts(n, bd)
    tmp = (block @ m.T + (1 << (s1 - 1))) >> s1               # partialButterfly over the rows
    out = (m @ tmp + (1 << (s2 - 1))) >> s2                   # ... over the columns
    return (tmp, out) if stages else out


def quant(n, bd, qp):
    """-> (scale, qbits, add_plain, add_half) of an n x n TU"""
    qpp = qp + 6 * (bd - 8)
    per, rem = qpp // 6, qpp % 6
    qbits = 14 + per + (15 - bd - log2(n))
    return QUANT_SCALES[rem], qbits, 85 << (qbits - 9), 1 << (qbits - 1)


def level(c, scale, qbits, add):
    return (abs(int(c)) * scale + add) >> qbits


def first_nonzero(n, bd, qp, half):
    """the smallest |c| whose level is 1, from the formula: (c * scale + add) >> qbits >= 1 iff c * scale >= 2^qbits - add"""
    scale, qbits, add_plain, add_half = quant(n, bd, qp)
    need = (1 << qbits) - (add_half if half else add_plain)
    return -(-need // scale)


def coefficients(res, bd):
    """all coefficients of a node's TU or TUs, int64, flat"""
    res = np.asarray(res, np.int64)
    s = res.shape[0]
    n = min(s, 32)
    return np.concatenate([forward(res[y:y + n, x:x + n], bd).reshape(-1) for y in range(0, s, n) for x in range(0, s, n)])


def node_record(res, bd, qp, mv=(0, 0)):
    """res: the s x s residual of a node -> the record tuple (coef_max, level_sum, nonzero, flags, pad, mvx, mvy); int64 throughout: |c| * scale + add
    stays below 2^31"""
    scale, qbits, add_plain, add_half = quant(min(np.asarray(res).shape[0], 32), bd, qp)
    mags = np.abs(coefficients(res, bd))
    levels = (mags * scale + add_plain) >> qbits
    nonzero = int((levels != 0).sum())
    half_zero = not (((mags * scale + add_half) >> qbits) != 0).any()
    return (int(mags.max()), int(levels.sum()), nonzero, (ZERO_PLAIN if nonzero == 0 else 0) | (ZERO_HALF if half_zero else 0), 0, mv[0], mv[1])


def node_record_loop(res, bd, qp, mv=(0, 0)):
    """node_record, one coefficient at a time in Python integers"""
    scale, qbits, add_plain, add_half = quant(min(np.asarray(res).shape[0], 32), bd, qp)
    top = total = nonzero = half_nonzero = 0
    for c in coefficients(res, bd).tolist():
        lv = level(c, scale, qbits, add_plain)
        top, total, nonzero = max(top, abs(c)), total + lv, nonzero + (1 if lv else 0)
        half_nonzero += 1 if level(c, scale, qbits, add_half) else 0
    return (top, total, nonzero, (ZERO_PLAIN if nonzero == 0 else 0) | (ZERO_HALF if half_nonzero == 0 else 0), 0, mv[0], mv[1])


def residual(planes, cur, x0, y0, n, q):
    """original minus fhevc_motion_refine's prediction of the n x n node at (x0, y0) at q = (qx, qy) quarter samples; cur: the picture [H, W]"""
    return np.asarray(cur, np.int64)[y0:y0 + n, x0:x0 + n] - planes.block(q[0], q[1], x0, y0, n).astype(np.int64)


def expected(cur, ref_pic, W, H, bd, qp, merge, max_range, rows=None, planes=None):
    """cur / ref_pic: the samples [H, W]; merge: [band CTUs, 85] MOTION_MERGE_DTYPE (cost_best, mvx, mvy are read), compact over the CTU rows `rows`
    -> [band CTUs, 85] MOTION_SKIP_DTYPE"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    merge = merge.reshape(nb, 85)
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    assert planes.pad >= max_range + 6 and planes.bd == bd
    reach = 4 * max_range + 3
    out = np.zeros((nb, 85), SDT)
    for i in range(nb):
        c = rows[0] * cw + i
        cx, cy = c % cw, c // cw
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            n = 64 >> lvl
            x0, y0 = cx * 64 + bx * n, cy * 64 + by * n
            q = (int(merge["mvx"][i, k]), int(merge["mvy"][i, k]))
            if x0 + n > W or y0 + n > H or int(merge["cost_best"][i, k]) == MARK or abs(q[0]) > reach or abs(q[1]) > reach:
                out[i, k] = INVALID
            else:
                out[i, k] = node_record(residual(planes, cur, x0, y0, n, q), bd, qp, q)
    return out


def same(got, exp, what=""):
    """every byte of every record"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    for f in SDT.names:
        bad = got[f] != exp[f]
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())


# ---- the tree decision with the skip answer: the merge tree with HM's EarlyCU --------------------------------------------------------------------

def tree_ctu(shape_cost, merge_cost, skip_flags, skip_mask, valid_w, valid_h, rule=None):
    """one CTU: cost_best of the 85 selection and merge records, flags of the 85 skip records -> (records [85] TREE_DTYPE, depth_min, depth_max [256]).
    An INSIDE node of level 0..2 whose own cost is the merge cost and whose skip flags carry a masked bit is not descended: tree = own, stop_sure,
    bit 7."""
    R = pt.rule_fields(rule)
    own, kids, tree, flags = [MARK] * 85, [MARK] * 85, [MARK] * 85, [0] * 85
    sure, maybe = [False] * 21, [True] * 21
    for k in range(84, -1, -1):
        l = pt.level(k)
        inside, outside, crossing, absent = pt.geometry(k, valid_w, valid_h)
        if absent:
            flags[k] = pt.ABSENT
            continue
        sc, mc = int(shape_cost[k]), int(merge_cost[k])
        merged = inside and mc < sc
        own[k] = (mc if merged else sc) if inside else MARK
        if l == 3:
            tree[k] = own[k]
        else:
            coded = [c for c in pt.children(k) if not pt.geometry(c, valid_w, valid_h)[3]]
            if not any(tree[c] == MARK for c in coded):
                kids[k] = min(sum(tree[c] for c in coded) + (R["split_cost"][l] if inside else 0), pt.SAT)
            if crossing:
                tree[k] = kids[k]
            elif kids[k] == MARK:
                tree[k] = own[k]
            elif own[k] == MARK:
                tree[k] = kids[k]
            else:
                tree[k] = kids[k] if kids[k] < own[k] else own[k]
            split = stop = False
            if inside and own[k] != MARK and kids[k] != MARK:
                split = kids[k] + R["split_abs"][l] + ((kids[k] * R["split_q8"][l]) >> 8) < own[k]
                stop = own[k] + R["stop_abs"][l] + ((own[k] * R["stop_q8"][l]) >> 8) <= kids[k]
            if merged and int(skip_flags[k]) & skip_mask:
                tree[k], split, stop = own[k], False, True
                flags[k] |= SKIPPED
            sure[k] = crossing or split
            maybe[k] = crossing or not stop
            flags[k] |= (pt.SPLIT_SURE if split else 0) | (pt.STOP_SURE if stop else 0) | (pt.CROSSING if crossing else 0)
        flags[k] |= (pt.OWN_AVAILABLE if own[k] != MARK else 0) | (pt.KIDS_AVAILABLE if kids[k] != MARK else 0) | (mg.MERGED if merged else 0)
    rec = np.zeros(85, pt.TDT)
    rec["cost_own"], rec["cost_kids"], rec["cost_tree"], rec["flags"] = own, kids, tree, flags
    rec["level"] = [pt.level(k) for k in range(85)]
    dmin, dmax = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    for uy in range(16):
        for ux in range(16):
            if 4 * ux >= valid_w or 4 * uy >= valid_h:
                continue
            lo = hi = 0
            lo_open = hi_open = True
            for l in range(3):
                k = pt.node_id(l, ux >> (4 - l), uy >> (4 - l))
                lo_open, hi_open = lo_open and sure[k], hi_open and maybe[k]
                lo, hi = (l + 1 if lo_open else lo), (l + 1 if hi_open else hi)
            dmin[uy * 16 + ux], dmax[uy * 16 + ux] = lo, hi
    return rec, dmin, dmax


def tree_select(shapes, merge, skip, skip_mask, W, H, rows=None, rule=None):
    """shapes / merge / skip: [P, band CTUs, 85] records -> (records, depth_min, depth_max) as p_tree_ref.select"""
    sc, mc, sf = shapes["cost_best"], merge["cost_best"], skip["flags"]
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rb, re = rows if rows is not None else (0, ch)
    P, nb = sc.shape[:2]
    assert nb == (re - rb) * cw
    rec, dmin, dmax = np.zeros((P, nb, 85), pt.TDT), np.zeros((P, nb, 256), np.uint8), np.zeros((P, nb, 256), np.uint8)
    for p in range(P):
        for i in range(nb):
            rec[p, i], dmin[p, i], dmax[p, i] = tree_ctu(sc[p, i], mc[p, i], sf[p, i], skip_mask, *pt.valid_size(rb * cw + i, W, H), rule)
    return rec, dmin, dmax


def random_skip(rng, shape):
    """skip records of the given shape: every byte random -- only flags may matter --, flags drawn evenly from 0..3 and, a quarter of the time, with
    random high bits on top (which no mask may read)"""
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), SDT).reshape(shape).copy()
    f = rng.integers(0, 4, size=shape).astype(np.uint8)
    a["flags"] = np.where(rng.random(shape) < 0.25, f | (rng.integers(0, 64, size=shape).astype(np.uint8) << 2), f)
    return a


def flag_coverage(skip, merged_inside):
    """per level 0..2 the set of (flags & 3) values seen on nodes whose own cost is the merge cost; merged_inside: bool [..., 85]"""
    f = (skip["flags"] & 3).reshape(-1, 85)
    m = np.asarray(merged_inside).reshape(-1, 85)
    return {l: set(f[:, [k for k in range(21) if pt.level(k) == l]][m[:, [k for k in range(21) if pt.level(k) == l]]].tolist()) for l in range(3)}


# ---- constructed cases whose answers are known in advance (the CPU test confirms them, the GPU test runs the device on them) -------------------------------

FLAT_CASES = [(8, 1), (10, 5)]          # bit depth, offset d


def flat_offset_expectation(bd, d):
    """cur = ref + d on a flat field, zero vectors: the only non-zero coefficient of every TU is its DC = d << (15 - bd) -> per level 0..3 the two sets of
    QPs at which bit 0 and bit 1 are set, from the thresholds alone"""
    c = d << (15 - bd)
    return {lvl: tuple({qp for qp in range(52) if c < first_nonzero(min(64 >> lvl, 32), bd, qp, half)} for half in (False, True)) for lvl in range(4)}


def root_skip_case():
    """one whole CTU in which the children are cheaper than the root (kids = 40 < own), the root's own cost is its merge cost, and the root's skip record
    carries bit 1 -> (shapes, merge, skip) [1, 1, 85]"""
    shapes, merge, skip = np.zeros((1, 1, 85), capi.SHAPE_DTYPE), np.zeros((1, 1, 85), mg.MDT), np.zeros((1, 1, 85), SDT)
    shapes["cost_best"], merge["cost_best"] = 10, MARK
    shapes["cost_best"][0, 0, 0], merge["cost_best"][0, 0, 0] = 100000, 90000
    skip["flags"][0, 0, 0] = ZERO_HALF
    return shapes, merge, skip
