"""The partition-size selection (fhevc_pu_shape_select*), restated in numpy from the definition in include/fasthevc.h -- not from the C code.
tests/test_pu_shape_ref.py holds this module to hand-computed cases without a GPU; tests/test_pu_shape_abi.py compares the host function with it,
tests/test_gpu_pu_shape.py the kernel.  Python integers throughout (no 32-bit wrap can hide here).  A plain module, not a conftest and not a test."""
import numpy as np

from fasthevc_amd import capi

MARKER = 0xFFFFFFFF
SATURATED = 0xFFFFFFFE
ORDER = (0, 2, 1, 4, 5, 6, 7)          # HM's checking order: 2Nx2N, Nx2N, 2NxN, then the AMP pairs
LEVEL_FIRST = (0, 1, 5, 21)
SDT = capi.SHAPE_DTYPE


def level(k):
    return 0 if k < 1 else (1 if k < 5 else (2 if k < 21 else 3))


def node_rect(k):
    """(x, y, size) of node k inside its CTU"""
    l = level(k)
    i, n = k - LEVEL_FIRST[l], 64 >> l
    return (i % (1 << l)) * n, (i // (1 << l)) * n, n


def shape_of(p):
    """the library's shape number of partition size p (1, 2, 4..7)"""
    return p - 1 if p <= 2 else p - 2


def parts(k, p):
    """(family, entry of part 0, entry of part 1) of partition size p of node k: family "pu" (the 124) or "small" (the 384); None: not covered"""
    if p in (0, 3):
        return None
    s = shape_of(p)
    if k < 5:
        e = k * 12 + s * 2
        return "pu", e, e + 1
    if k < 21:
        if p <= 2:
            e = 60 + (k - 5) * 4 + s * 2
            return "pu", e, e + 1
        e = (k - 5) * 8 + (s - 2) * 2
        return "small", e, e + 1
    if p <= 2:
        e = 128 + (k - 21) * 4 + s * 2
        return "small", e, e + 1
    return None          # HM opens AMP only above the smallest CU


def cost_table(nodes, pus, pus_small, valid_w=64, valid_h=64):
    """one CTU: cost_best of the 85 / 124 / 384 (or None) refined entries -> 85 x 8 list of Python ints"""
    out = []
    for k in range(85):
        x, y, n = node_rect(k)
        row = [MARKER] * 8
        if x + n <= valid_w and y + n <= valid_h:
            row[0] = int(nodes[k])
            for p in (1, 2, 4, 5, 6, 7):
                w = parts(k, p)
                if w is None:
                    continue
                src = pus if w[0] == "pu" else pus_small
                if src is None:
                    continue
                a, b = int(src[w[1]]), int(src[w[2]])
                if a != MARKER and b != MARKER:
                    row[p] = min(a + b, SATURATED)
        out.append(row)
    return out


def scan(row, skip=None):
    """(cost, partition size) of the smallest available cost in HM's checking order, strict "<"; (MARKER, 255) if none"""
    best, cost = 255, MARKER
    for p in ORDER:
        if p == skip or row[p] == MARKER:
            continue
        if best == 255 or row[p] < cost:
            best, cost = p, row[p]
    return cost, best


def select_node(row, lvl, valid, margin_q8, margin_abs, amp_mode):
    """one node: its eight costs -> (cost_2Nx2N, cost_best, cost_second, best, second, mask, avail)"""
    if not valid:
        return MARKER, MARKER, MARKER, 255, 255, 0, 0
    avail = sum(1 << p for p in range(8) if row[p] != MARKER)
    cost_best, best = scan(row)
    cost_second, second = scan(row, skip=best) if best != 255 else (MARKER, 255)
    mask = 1
    if best != 255:
        limit = cost_best + margin_abs[lvl] + ((cost_best * margin_q8[lvl]) >> 8)
        for p in range(8):
            if row[p] != MARKER and row[p] <= limit:
                mask |= 1 << p
    if amp_mode == 1:
        _, b3 = scan([row[p] if p in (0, 1, 2) else MARKER for p in range(8)])
        if b3 not in (0, 1):
            mask &= ~0x30
        if b3 not in (0, 2):
            mask &= ~0xC0
    return row[0], cost_best, cost_second, best, second, mask, avail


def rule_fields(rule):
    """a capi.PuShapeRule (or None: the documented default) -> (margin_q8[4], margin_abs[4], amp_mode)"""
    if rule is None:
        return [0] * 4, [0] * 4, 1
    return list(rule.margin_q8), list(rule.margin_abs), int(rule.amp_mode)


def select_ctu(nodes, pus, pus_small, valid_w, valid_h, rule=None):
    """one CTU: cost_best arrays of the refined entries -> (records [85] SHAPE_DTYPE, costs [85, 8] uint32)"""
    q8, ab, amp = rule_fields(rule)
    table = cost_table(nodes, pus, pus_small, valid_w, valid_h)
    rec = np.zeros(85, SDT)
    for k in range(85):
        x, y, n = node_rect(k)
        rec[k] = select_node(table[k], level(k), x + n <= valid_w and y + n <= valid_h, q8, ab, amp)
    return rec, np.array(table, np.uint64).astype(np.uint32)


def select(nodes, pus, pus_small, W, H, rows=None, rule=None):
    """nodes [P, band CTUs, 85], pus [P, band CTUs, 124], pus_small [P, band CTUs, 384] or None: arrays with a cost_best field (or plain integer
    arrays of cost_best), compact over CTU rows `rows` of a W x H picture -> (records [P, band CTUs, 85], costs [P, band CTUs, 85, 8])"""
    cb = lambda a: None if a is None else (a["cost_best"] if a.dtype.names else a)
    nodes, pus, pus_small = cb(nodes), cb(pus), cb(pus_small)
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rb, re = rows if rows is not None else (0, ch)
    P, nb = nodes.shape[:2]
    assert nb == (re - rb) * cw
    rec, costs = np.zeros((P, nb, 85), SDT), np.zeros((P, nb, 85, 8), np.uint32)
    for p in range(P):
        for i in range(nb):
            ctu = rb * cw + i
            vw, vh = min(64, W - (ctu % cw) * 64), min(64, H - (ctu // cw) * 64)
            rec[p, i], costs[p, i] = select_ctu(nodes[p, i], pus[p, i], None if pus_small is None else pus_small[p, i], vw, vh, rule)
    return rec, costs


def same(got, exp, what=""):
    """every field of every record"""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    for f in SDT.names:
        bad = got[f] != exp[f]
        assert not bad.any(), (what, f, np.argwhere(bad)[:5], got[f][bad][:5], exp[f][bad][:5])


# ---- random inputs that make every case of the definition occur (shared by the ABI test and the GPU test) ------------------------------------------

def random_entries(rng, P, n):
    """(nodes [P, n, 85], pus [P, n, 124], pus_small [P, n, 384]) of MOTION_QPEL_DTYPE: cost_best from a few small values (ties), about 5 % markers, a
    few values near 2^32 (saturation, no 32-bit wrap in the margin); the other fields random -- only cost_best may matter"""
    out = []
    for per in (85, 124, 384):
        a = np.zeros((P, n, per), capi.MOTION_QPEL_DTYPE)
        c = rng.choice(np.array([100, 100, 101, 120, 150, 200, 256, 1000], np.uint32), size=(P, n, per))
        u = rng.random((P, n, per))
        c[u < 0.05] = MARKER
        big = (u >= 0.05) & (u < 0.09)
        c[big] = rng.choice(np.array([0xFFFFFFF0, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF, 0xFFFFFF00], np.uint32), size=int(big.sum()))
        a["cost_best"] = c
        a["satd_int"] = rng.integers(0, 1 << 32, size=c.shape, dtype=np.uint64).astype(np.uint32)
        a["satd_best"] = rng.integers(0, 1 << 32, size=c.shape, dtype=np.uint64).astype(np.uint32)
        a["mvx"] = rng.integers(-260, 260, size=c.shape)
        a["mvy"] = rng.integers(-260, 260, size=c.shape)
        out.append(a)
    return tuple(out)


def random_rule(rng, amp_mode):
    q8 = [int(v) for v in rng.choice([0, 1, 13, 64, 256, 65535], size=4)]
    ab = [int(v) for v in rng.choice([0, 1, 20, 100, 0x7FFFFFFF], size=4)]
    return capi.pu_shape_rule(q8, ab, amp_mode)
