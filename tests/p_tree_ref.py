"""The tree decision (fhevc_p_tree_select*), restated in Python from the definition in include/fasthevc.h -- not from the C code.
tests/test_p_tree_ref.py holds this module to hand-computed cases without a GPU; tests/test_p_tree_abi.py compares the host function with it,
tests/test_gpu_p_tree.py the kernel.  Python integers throughout (no 32-bit wrap can hide here).  A plain module, not a conftest and not a test."""
import numpy as np

from fasthevc_amd import capi

MARK = 0xFFFFFFFF
SAT = 0xFFFFFFFE
LEVEL_FIRST = (0, 1, 5, 21)
TDT = capi.TREE_DTYPE
SPLIT_SURE, STOP_SURE, CROSSING, ABSENT, OWN_AVAILABLE, KIDS_AVAILABLE = 1, 2, 4, 8, 16, 32


def level(k):
    return 0 if k < 1 else (1 if k < 5 else (2 if k < 21 else 3))


def node_id(l, nx, ny):
    return LEVEL_FIRST[l] + ny * (1 << l) + nx


def node_pos(k):
    """(level, nx, ny) of node k"""
    l = level(k)
    i = k - LEVEL_FIRST[l]
    return l, i % (1 << l), i // (1 << l)


def geometry(k, valid_w, valid_h):
    """(inside, outside, crossing, absent) of node k"""
    l, nx, ny = node_pos(k)
    s = 64 >> l
    inside = nx * s + s <= valid_w and ny * s + s <= valid_h
    outside = nx * s >= valid_w or ny * s >= valid_h
    crossing = not inside and not outside
    return inside, outside, crossing, outside or (l == 3 and not inside)


def children(k):
    l, nx, ny = node_pos(k)
    return [node_id(l + 1, 2 * nx + dx, 2 * ny + dy) for dy in (0, 1) for dx in (0, 1)]


def rule_fields(rule):
    """a capi.PTreeRule (or None: the documented default, all zero) -> dict of five lists of three"""
    names = ("split_q8", "split_abs", "stop_q8", "stop_abs", "split_cost")
    if rule is None:
        return {n: [0, 0, 0] for n in names}
    return {n: [int(v) for v in getattr(rule, n)] for n in names}


def tree_ctu(cost_best, valid_w, valid_h, rule=None):
    """one CTU: cost_best of its 85 records -> (records [85] TREE_DTYPE, depth_min [256], depth_max [256])"""
    R = rule_fields(rule)
    own, kids, tree, flags = [MARK] * 85, [MARK] * 85, [MARK] * 85, [0] * 85
    sure, maybe = [False] * 21, [True] * 21
    for k in range(84, -1, -1):
        l = level(k)
        inside, outside, crossing, absent = geometry(k, valid_w, valid_h)
        if absent:
            flags[k] = ABSENT
            continue
        own[k] = int(cost_best[k]) if inside else MARK
        if l == 3:
            tree[k] = own[k]
        else:
            coded = [c for c in children(k) if not geometry(c, valid_w, valid_h)[3]]
            if not any(tree[c] == MARK for c in coded):
                kids[k] = min(sum(tree[c] for c in coded) + (R["split_cost"][l] if inside else 0), SAT)
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
            sure[k] = crossing or split
            maybe[k] = crossing or not stop
            flags[k] = (SPLIT_SURE if split else 0) | (STOP_SURE if stop else 0) | (CROSSING if crossing else 0)
        flags[k] |= (OWN_AVAILABLE if own[k] != MARK else 0) | (KIDS_AVAILABLE if kids[k] != MARK else 0)
    rec = np.zeros(85, TDT)
    rec["cost_own"], rec["cost_kids"], rec["cost_tree"], rec["flags"] = own, kids, tree, flags
    rec["level"] = [level(k) for k in range(85)]
    dmin, dmax = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    for uy in range(16):
        for ux in range(16):
            if 4 * ux >= valid_w or 4 * uy >= valid_h:
                continue
            lo = hi = 0
            lo_open = hi_open = True
            for l in range(3):
                k = node_id(l, ux >> (4 - l), uy >> (4 - l))
                lo_open, hi_open = lo_open and sure[k], hi_open and maybe[k]
                lo, hi = (l + 1 if lo_open else lo), (l + 1 if hi_open else hi)
            dmin[uy * 16 + ux], dmax[uy * 16 + ux] = lo, hi
    return rec, dmin, dmax


def valid_size(ctu, W, H):
    cw = (W + 63) // 64
    return min(64, W - (ctu % cw) * 64), min(64, H - (ctu // cw) * 64)


def select(shapes, W, H, rows=None, rule=None):
    """shapes [P, band CTUs, 85]: SHAPE_DTYPE records (or plain integer arrays of cost_best), compact over CTU rows `rows` of a W x H picture ->
    (records [P, band CTUs, 85], depth_min [P, band CTUs, 256], depth_max [P, band CTUs, 256])"""
    cb = shapes["cost_best"] if shapes.dtype.names else shapes
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rb, re = rows if rows is not None else (0, ch)
    P, nb = cb.shape[:2]
    assert nb == (re - rb) * cw
    rec, dmin, dmax = np.zeros((P, nb, 85), TDT), np.zeros((P, nb, 256), np.uint8), np.zeros((P, nb, 256), np.uint8)
    for p in range(P):
        for i in range(nb):
            rec[p, i], dmin[p, i], dmax[p, i] = tree_ctu(cb[p, i], *valid_size(rb * cw + i, W, H), rule)
    return rec, dmin, dmax


def same(got, exp, what=""):
    """every byte of every record"""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    for f in TDT.names:
        bad = got[f] != exp[f]
        assert not bad.any(), (what, f, np.argwhere(bad)[:5], got[f][bad][:5], exp[f][bad][:5])


# ---- random inputs that make every case of the definition occur (shared by the ABI test and the GPU test) ------------------------------------------

def random_shapes(rng, P, n):
    """[P, n, 85] SHAPE_DTYPE.  cost_best per CTU in one of five styles drawn per CTU, so that every case occurs at every level: 0 children that add up
    to about their parent (splits and stops by a hair and -- where a rule has margins -- neither); 1 the same with markers: a few anywhere, and one chain
    of them from a leaf upwards (a marker that reaches a parent's sum needs every node below it marked); 2 values near 2^32 throughout (saturated
    sums); 3 plain small values; 4 every node exactly the sum of its children (ties at every level).  Every other byte of a record is random -- only
    cost_best may matter"""
    a = np.frombuffer(rng.bytes(P * n * 85 * 16), capi.SHAPE_DTYPE).reshape(P, n, 85).copy()
    c = np.zeros((P, n, 85), np.uint32)
    for p in range(P):
        for i in range(n):
            style = int(rng.integers(0, 5))
            if style == 2:
                v = rng.choice(np.array([0xFFFFFFF0, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF, 0x40000000, 0xFFFFFF00], np.uint32), size=85)
            elif style == 3:
                v = rng.choice(np.array([100, 100, 101, 120, 150, 200, 256, 1000], np.uint32), size=85)
            else:
                v = np.zeros(85, np.int64)
                v[21:] = rng.integers(100, 104, size=64)
                for k in range(20, -1, -1):
                    v[k] = sum(v[ch] for ch in children(k)) + (0 if style == 4 else int(rng.choice([-40, -3, -1, 0, 0, 0, 1, 3, 40])))
                v = v.astype(np.uint32)
            if style == 1:
                v = v.copy()
                v[rng.random(85) < 0.03] = MARK
                ux, uy = (int(t) for t in rng.integers(0, 8, size=2))
                chain = [node_id(3, ux, uy), node_id(2, ux >> 1, uy >> 1), node_id(1, ux >> 2, uy >> 2), 0]
                v[chain[:int(rng.integers(1, 5))]] = MARK
            c[p, i] = v
    a["cost_best"] = c
    return a


def random_rule(rng):
    pick = lambda values: [int(v) for v in rng.choice(values, size=3)]
    return capi.p_tree_rule(pick([0, 1, 13, 64, 256, 65535]), pick([0, 1, 20, 100, 0x7FFFFFFF]), pick([0, 1, 13, 64, 256, 65535]), pick([0, 1, 20, 100, 0x7FFFFFFF]),
                            pick([0, 0, 1, 7, 50, 0x7FFFFFFF]))


CASES = ("split_sure", "stop_sure", "neither", "own_mark", "kids_mark", "saturated", "tie", "crossing", "absent")


def coverage(rec, seen=None):
    """which cases of the definition the records [..., 85] show, per level 0..2 -> {case: set of levels}"""
    seen = seen if seen is not None else {c: set() for c in CASES}
    f, own, kids = rec["flags"].reshape(-1, 85), rec["cost_own"].reshape(-1, 85), rec["cost_kids"].reshape(-1, 85)
    coded = (f & (CROSSING | ABSENT)) == 0
    both = (f & (OWN_AVAILABLE | KIDS_AVAILABLE)) == (OWN_AVAILABLE | KIDS_AVAILABLE)
    shows = {"split_sure": f & SPLIT_SURE != 0, "stop_sure": f & STOP_SURE != 0, "neither": coded & both & (f & (SPLIT_SURE | STOP_SURE) == 0),
             "own_mark": coded & (f & OWN_AVAILABLE == 0), "kids_mark": coded & (f & KIDS_AVAILABLE == 0), "saturated": kids == SAT,
             "tie": coded & both & (own == kids), "crossing": f & CROSSING != 0, "absent": f & ABSENT != 0}
    for case, hit in shows.items():
        seen[case] |= {level(k) for k in np.flatnonzero(hit[:, :21].any(axis=0))}
    return seen


def covers_everything(seen):
    """every case at every level 0..2 -- but for an ABSENT root, which the definition excludes (node (0, 0) of level 0 is never OUTSIDE)"""
    return all(seen[c] == ({1, 2} if c == "absent" else {0, 1, 2}) for c in CASES)
