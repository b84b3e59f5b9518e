"""Expected values of the RD estimate of the intra candidate (fhevc_intra_rd*), restated from the definition in include/fasthevc.h -- not from the C code:
per TU the oracle's four intra functions (fho_fill_ref -> fho_filter_ref -> fho_use_filtered_ref -> fho_pred_intra, through oracle_py; these are what the
first pass is pinned to) composed with motion_rd_ref's TU arithmetic (forward transform, plain quantiser, xDeQuant, inverse transform, xGetSSE, the bit
estimate; pinned to the reference's own by tests/test_motion_rd_ref.py), then the intra choice rule, the calm gate and the fold.  The composition itself
rests on this module alone: HM's own intra coding predicts from reconstructed neighbours and cannot pin it.  tests/test_intra_rd_ref.py holds the module
to closed forms without a GPU; tests/test_gpu_intra_rd.py compares the library with it.  A plain module, not a conftest and not a test."""
import functools

import numpy as np

import motion_rd_ref as rd
import motion_refine_ref as mr
from fasthevc_amd import capi

MARK, SAT = rd.MARK, rd.SAT
PDT, NDT, RDT = capi.MOTION_RD_PU_DTYPE, capi.NODE_DTYPE, capi.MOTION_RD_DTYPE
PART_INTRA = capi.RD_PART_INTRA
ZERO_PLAIN, ZERO_HALF, TU_SPLIT = rd.ZERO_PLAIN, rd.ZERO_HALF, rd.TU_SPLIT
MARKER = np.array([(MARK, MARK, 0xFFFF, 0, 0, 255, 0, (0, 0))], PDT)[0]
LEVEL_OF = np.array([mr.node_geometry(k)[0] for k in range(85)])


def mode_bits(m):
    """bits(m) of fhevc_intra_p"""
    return 2 if m == 0 else (3 if m in (1, 26) else 6)


@functools.lru_cache(maxsize=1)
def oracle():
    from oracle import oracle_py as op
    return op.load_oracle(), op


class Picture:
    """one picture [H, W] at bd bits: the lines of a TU (once per TU) and its prediction at a mode, both from the oracle"""

    def __init__(self, pic, bd):
        self.lib, self.op = oracle()
        self.pic = np.asarray(pic, np.int64)
        self.H, self.W = self.pic.shape
        self.bd = bd
        self.flat = np.ascontiguousarray(self.pic.astype(np.int16)).reshape(-1)
        self.lines = {}
        self.filtered = {}   # (n, decision) -> how often a prediction was taken from the smoothed / the plain line

    def predict(self, x0, y0, n, mode):
        key = (x0, y0, n)
        if key not in self.lines:
            ref, flt = np.zeros(4 * n + 1, np.int16), np.zeros(4 * n + 1, np.int16)
            self.lib.fho_fill_ref(self.op.ptr(self.flat, 0), self.W, self.W, self.H, x0, y0, n, self.bd, ref)
            self.lib.fho_filter_ref(ref, n, self.bd, 1, flt)
            self.lines[key] = (ref, flt)
        ref, flt = self.lines[key]
        use = int(self.lib.fho_use_filtered_ref(mode, n))
        self.filtered[(n, use)] = self.filtered.get((n, use), 0) + 1
        pred = np.zeros(n * n, np.int16)
        self.lib.fho_pred_intra(ref, flt, n, mode, self.bd, pred)   # takes the line fho_use_filtered_ref names
        return pred.reshape(n, n).astype(np.int64)

    def node(self, x0, y0, s, mode):
        """the node's prediction assembled from its depth-0 TUs and from its depth-1 TUs (None for an 8x8 node) -> ([s, s], [s, s] or None)"""
        n0 = min(s, 32)
        out = []
        for n in (n0, n0 // 2):
            if n < 8:
                out.append(None)
                continue
            p = np.zeros((s, s), np.int64)
            for ty in range(0, s, n):
                for tx in range(0, s, n):
                    p[ty:ty + n, tx:tx + n] = self.predict(x0 + tx, y0 + ty, n, mode)
            out.append(p)
        return out


def tu_choice(d0, r0, d1, r1, lam):
    """one depth-0 TU against its four children (their sums) -> (J0, J1, split taken): dSplitCost < dSingleCost alone (TEncSearch.cpp:1661), strictly"""
    j0 = 256 * np.asarray(d0, np.int64) + lam * (1 + np.asarray(r0, np.int64))
    j1 = 256 * np.asarray(d1, np.int64) + lam * (1 + np.asarray(r1, np.int64))
    return j0, j1, j1 < j0


def node_records(org, pred0, pred1, bd, qp, side, detail=None):
    """org, pred0 [M, s, s], pred1 [M, s, s] or None (8x8 nodes), side [M] -> (dist, cost_rd, bits, flags, tu_split) arrays [M]"""
    s = org.shape[-1]
    n0 = min(s, 32)
    lam = rd.lam_q8(qp)
    o0 = rd.split(np.asarray(org, np.int64), n0)
    a = rd.tu_pass(o0, rd.split(np.asarray(pred0, np.int64), n0), bd, qp)
    if pred1 is not None:
        b = rd.tu_pass(rd.split(o0, n0 // 2), rd.split(rd.split(np.asarray(pred1, np.int64), n0), n0 // 2), bd, qp)
        d1, r1, any1, clip1 = b["D"].sum(axis=-1), b["r"].sum(axis=-1), b["cbf"].any(axis=-1), b["clipped"].sum(axis=-1)
        j0, j1, take = tu_choice(a["D"], a["r"], d1, r1, lam)
    else:
        d1 = r1 = clip1 = np.zeros_like(a["D"])
        any1 = np.zeros(a["D"].shape, bool)
        j0, j1, take = tu_choice(a["D"], a["r"], d1, r1, lam)
        take = np.zeros_like(take)
    side = np.asarray(side, np.int64)
    j = np.where(take, j1, j0).sum(axis=-1) + lam * side
    dist = np.where(take, d1, a["D"]).sum(axis=-1)
    bits = (1 + np.where(take, r1, a["r"])).sum(axis=-1) + side
    flags = np.where(~a["cbf"].any(axis=-1), ZERO_PLAIN, 0) | np.where(a["zero_half"].all(axis=-1), ZERO_HALF, 0) | np.where(take.any(axis=-1), TU_SPLIT, 0)
    tu_split = (take.astype(np.int64) << np.arange(take.shape[-1])).sum(axis=-1)
    if detail is not None:
        detail.update(J0=j0, J1=j1, take=take, any1=any1, D0=a["D"], D1=d1, clipped=a["clipped"] + clip1, has_depth1=pred1 is not None)
    return dist, np.minimum(j >> 8, SAT), np.minimum(bits, 65535), flags, tu_split


class Stats:
    """what a draw exercised, per level 0..3"""
    KEYS = ("taken", "not_taken", "taken_uncoded", "clipped", "negative", "dc", "planar", "vertical", "horizontal")

    def __init__(self):
        self.n = {k: [0, 0, 0, 0] for k in self.KEYS}
        self.modes = [set(), set(), set(), set()]
        self.filtered = {}

    def add(self, lvl, detail, modes):
        t = detail["take"]
        if detail["has_depth1"]:
            self.n["taken"][lvl] += int(t.sum())
            self.n["not_taken"][lvl] += int((~t).sum())
            self.n["taken_uncoded"][lvl] += int((t & ~detail["any1"]).sum())
        self.n["clipped"][lvl] += int((detail["clipped"] > 0).sum())
        m = np.asarray(modes)
        for k, sel in (("negative", (m > 10) & (m < 26)), ("dc", m == 1), ("planar", m == 0), ("vertical", m == 26), ("horizontal", m == 10)):
            self.n[k][lvl] += int(sel.sum())
        self.modes[lvl] |= set(int(x) for x in m)


def plain(pic, bd, qp, first, rows=None, stats=None):
    """pic [H, W], first [band CTUs, 85] NODE_DTYPE (any bytes) -> the plain intra RD records [band CTUs, 85] MOTION_RD_PU_DTYPE"""
    P = pic if isinstance(pic, Picture) else Picture(pic, bd)
    W, H = P.W, P.H
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    first = first.reshape(nb, 85)
    out = np.zeros((nb, 85), PDT)
    out[:] = MARKER
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
            p0, p1 = P.node(x0, y0, s, mode)
            todo[lvl].append((i, k, P.pic[y0:y0 + s, x0:x0 + s], p0, p1, mode))
    for lvl, items in todo.items():
        if not items:
            continue
        detail = {} if stats is not None else None
        p1 = np.stack([t[4] for t in items]) if lvl < 3 else None
        dist, cost, bits, flags, tus = node_records(np.stack([t[2] for t in items]), np.stack([t[3] for t in items]), p1, bd, qp, [mode_bits(t[5]) for t in items], detail)
        for m, (i, k, _, _, _, mode) in enumerate(items):
            out[i, k] = (int(dist[m]), int(cost[m]), int(bits[m]), int(flags[m]), int(tus[m]), PART_INTRA, 0, (mode, 0))
        if stats is not None:
            stats.add(lvl, detail, [t[5] for t in items])
    if stats is not None:
        for k, v in P.filtered.items():
            stats.filtered[k] = stats.filtered.get(k, 0) + v
    return out


CALM, INTRA, KEPT, NO_FOLD = 0, 1, 2, 3


def gate_fold(intra, fold=None, rd_merge=None, skip_mask=0, outcome=None):
    """the calm gate and the fold on plain intra records (any shape) -> the records written; outcome: an int array of the same shape that takes CALM /
    INTRA (written over the fold record) / KEPT (the fold record stays) / NO_FOLD (the plain record, no fold given and not calm)"""
    fc = fold["cost_rd"].astype(np.int64) if fold is not None else np.full(intra.shape, MARK, np.int64)
    base = fold if fold is not None else np.full(intra.shape, MARKER, PDT)
    calm = np.zeros(intra.shape, bool)
    if rd_merge is not None:
        calm = (rd_merge["cost_rd"].astype(np.int64) < fc) & ((rd_merge["flags"] & skip_mask) != 0)
    valid = intra["part"] != 255
    wins = (valid & (intra["cost_rd"].astype(np.int64) < fc)) if fold is not None else np.ones(intra.shape, bool)
    out = np.where(~calm & wins, intra, base)
    if outcome is not None:
        outcome[...] = np.where(calm, CALM, np.where(fold is None, NO_FOLD, np.where(wins, INTRA, KEPT)))
    return out


def expected(pic, bd, qp, first, fold=None, rd_merge=None, skip_mask=0, rows=None, stats=None, outcome=None):
    """one picture -> [band CTUs, 85] MOTION_RD_PU_DTYPE; fold / rd_merge compact over the same rows, or None"""
    p = plain(pic, bd, qp, first, rows, stats)
    return gate_fold(p, None if fold is None else fold.reshape(p.shape), None if rd_merge is None else rd_merge.reshape(p.shape), skip_mask, outcome)


def same(got, exp, what=""):
    """every byte of every record"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    for f in PDT.names:
        bad = got[f] != exp[f]
        if bad.ndim > got.ndim:
            bad = bad.any(axis=-1)
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())


# ---- the draw: motion_rd_ref's 168 x 152 current pictures; modes from the real first pass or uniform over 0..34; records around the intra costs ---------------

DRAW_W, DRAW_H, DRAW_N, DRAW_QPS = rd.DRAW_W, rd.DRAW_H, rd.DRAW_N, rd.DRAW_QPS
# 35 pictures: every (bit depth, QP) pair once in the first 21, one picture in five with the real first pass's modes
DRAW = [((8, 10, 12)[i % 3], DRAW_QPS[i % 7], i, i % 5 == 0) for i in range(35)]


def draw_picture(bd, seed):
    return rd.draw_pictures(bd, seed)[1]


def first_pass(pic, bd, qp):
    """the oracle's first pass of a picture -> [numCtus, 85] NODE_DTYPE"""
    lib, op = oracle()
    H, W = pic.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    flat = np.ascontiguousarray(np.asarray(pic).astype(np.int16)).reshape(-1)
    sl = lib.fho_lambda_intra(qp, bd) ** 0.5
    first = np.zeros((cw * ch, 85), NDT)
    e85 = (op.NodeCost * 85)()
    for c in range(cw * ch):
        lib.fho_first_pass_ctu(op.ptr(flat, 0), W, W, H, c % cw, c // cw, bd, sl, e85)
        first[c] = np.frombuffer(e85, dtype=NDT)
    return first


def forced(modes, shape=(DRAW_N, 85)):
    """first-pass records that force a mode (a number or an array) on every node: satd 0, the other bytes zero"""
    a = np.zeros(shape, NDT)
    a["mode"] = modes
    return a


def draw_first(pic, bd, qp, seed, real):
    """real: the oracle's records with their high mode bytes filled (only the low byte counts); otherwise random bytes with modes uniform over 0..34 (four in ten: one of 0, 1, 10, 26), one in
    twelve beyond 34 and one in twelve with the marker satd"""
    rng = np.random.default_rng(7000 + seed)
    if real:
        a = first_pass(pic, bd, qp)
        inside = a["satd"] != MARK
        a["mode"] = np.where(inside, a["mode"] | (rng.integers(0, 1 << 24, size=a.shape) << 8).astype(np.uint32), a["mode"])
        return a
    a = np.frombuffer(rng.bytes(DRAW_N * 85 * 16), NDT).reshape(DRAW_N, 85).copy()
    kind = rng.random(a.shape)
    special = rng.choice([0, 1, 10, 26], size=a.shape)   # planar, DC and the two pure directions: the modes with edge filters, rare under a uniform draw
    mode = np.where(kind < 1 / 12, rng.integers(35, 256, size=a.shape), np.where(rng.random(a.shape) < 0.4, special, rng.integers(0, 35, size=a.shape)))
    a["mode"] = (a["mode"] & 0xFFFFFF00) | mode.astype(np.uint32)
    a["satd"] = np.where((kind >= 1 / 12) & (kind < 2 / 12), MARK, a["satd"] % 1000000)
    return a


def draw_inter(plain_records, seed):
    """fold and merge RD records around the plain intra costs, so that every outcome of gate and fold occurs: the fold record one less / equal / one more /
    far below / far above the intra cost or a marker, the merge record one less / equal / one more than the fold record or a marker, any flags"""
    rng = np.random.default_rng(8000 + seed)
    shape = plain_records.shape
    ic = np.where(plain_records["part"] == 255, rng.integers(1, 1 << 20, size=shape), plain_records["cost_rd"].astype(np.int64))
    fold = np.frombuffer(rng.bytes(plain_records.size * 16), PDT).reshape(shape).copy()
    delta = rng.choice([-1, 0, 1, -1000, 1000], size=shape)
    fold["cost_rd"] = np.clip(ic + delta, 0, SAT)
    fold["part"] = rng.choice([0, 1, 2, 4, 5, 6, 7], size=shape)
    gone = rng.random(shape) < 1 / 8
    fold[gone] = MARKER
    merge = np.frombuffer(rng.bytes(plain_records.size * 16), RDT).reshape(shape).copy()
    merge["cost_rd"] = np.clip(fold["cost_rd"].astype(np.int64) + rng.choice([-1, 0, 1], size=shape), 0, MARK)
    merge["cost_rd"] = np.where(rng.random(shape) < 1 / 8, MARK, merge["cost_rd"])
    merge["flags"] = rng.integers(0, 8, size=shape)
    return fold, merge


@functools.lru_cache(maxsize=None)
def draw(index):
    """entry `index` of DRAW -> dict: bd, qp, pic, first, plain (with stats), fold, merge"""
    bd, qp, seed, real = DRAW[index]
    pic = draw_picture(bd, seed)
    first = draw_first(pic, bd, qp, seed, real)
    stats = Stats()
    p = plain(pic, bd, qp, first, stats=stats)
    fold, merge = draw_inter(p, seed)
    return dict(bd=bd, qp=qp, pic=pic, first=first, plain=p, stats=stats, fold=fold, merge=merge)
