"""Expected values of the intra RD stage with the NxN candidate of the 8x8 nodes (fhevc_intra_rd_nxn*, fhevc_p_tree_rd_intra_nxn_frame), restated in numpy
from the definition in include/fasthevc.h -- not from the C code.  Everything but the candidate is intra_rd_qt_ref's at three TU depths: its tu_pass with
the DST prices the four 4x4 TUs, its `plain` gives the 2Nx2N records, intra_rd_ref's gate and fold act on the chosen record; the prediction of a PU is
intra_rd_ref.Picture.predict(x, y, 4, m_i).  tests/test_intra_rd_nxn_ref.py holds this module to closed forms without a GPU;
tests/test_gpu_intra_rd_nxn.py compares the library with it.  A plain module, not a conftest and not a test."""
import functools

import numpy as np

import first_pass_4x4_ref as fp4
import intra_rd_qt_ref as qt
import intra_rd_ref as ir
import motion_rd_ref as rd
import motion_refine_ref as mr
from fasthevc_amd import capi

MARK, SAT = rd.MARK, rd.SAT
PDT, NDT, XDT = capi.MOTION_RD_PU_DTYPE, capi.NODE_DTYPE, capi.INTRA_RD_NXN_DTYPE
PART_NXN = capi.RD_PART_INTRA_NXN
NXN_MARKER = np.array([(MARK, MARK, 0xFFFF, 0, 0, (255, 255, 255, 255))], XDT)[0]
NODE0, NODES8 = 21, 64   # the 8x8 nodes: 21..84, in 8x8 raster


def units(k):
    """the four PUs of 8x8 node 21 + k in fhevc_intra_p's order -> indices into the CTU's 16x16 raster of 4x4 units"""
    x, y = k % 8, k // 8
    return [(2 * y + (i >> 1)) * 16 + 2 * x + (i & 1) for i in range(4)]


def nxn_cost(D, r, side, lam):
    """D, r [..., 4] of the four TUs, side [...] = sum bits(m_i) -> (dist, cost_rd, bits): no split flag"""
    D, r, side = np.asarray(D, np.int64), np.asarray(r, np.int64), np.asarray(side, np.int64)
    bits = r.sum(axis=-1) + side
    j = 256 * D.sum(axis=-1) + lam * bits
    return D.sum(axis=-1), np.minimum(j >> 8, SAT), np.minimum(bits, 65535)


def candidates(pic, bd, qp, first4, rows=None, details=None):
    """pic [H, W] (or an intra_rd_ref.Picture), first4 [band CTUs, 256] NODE_DTYPE (any bytes) -> the plain NxN candidates [band CTUs, 64]
    INTRA_RD_NXN_DTYPE, the marker where the candidate is invalid; details: a dict that takes D, r [M, 4] and where [(ctu, k)]"""
    P = pic if isinstance(pic, ir.Picture) else ir.Picture(pic, bd)
    W, H = P.W, P.H
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    first4 = first4.reshape(nb, 256)
    out = np.zeros((nb, NODES8), XDT)
    out[:] = NXN_MARKER
    items = []
    for i in range(nb):
        c = rows[0] * cw + i
        cx, cy = c % cw, c // cw
        for k in range(NODES8):
            x0, y0 = cx * 64 + (k % 8) * 8, cy * 64 + (k // 8) * 8
            recs = first4[i, units(k)]
            modes = [int(m) & 0xFF for m in recs["mode"]]
            if x0 + 8 > W or y0 + 8 > H or any(int(s) == MARK for s in recs["satd"]) or any(m > 34 for m in modes):
                continue
            org = np.stack([P.pic[y0 + 4 * (j >> 1):y0 + 4 * (j >> 1) + 4, x0 + 4 * (j & 1):x0 + 4 * (j & 1) + 4] for j in range(4)])
            pred = np.stack([P.predict(x0 + 4 * (j & 1), y0 + 4 * (j >> 1), 4, modes[j]) for j in range(4)])
            items.append((i, k, org, pred, modes))
    if items:
        lam = rd.lam_q8(qp)
        t = qt.tu_pass(np.stack([it[2] for it in items]), np.stack([it[3] for it in items]), bd, qp)   # [M, 4, 4, 4] -> [M, 4]
        side = np.array([sum(ir.mode_bits(m) for m in it[4]) for it in items])
        dist, cost, bits = nxn_cost(t["D"], t["r"], side, lam)
        flags = np.where(~t["cbf"].any(axis=-1), rd.ZERO_PLAIN, 0) | np.where(t["zero_half"].all(axis=-1), rd.ZERO_HALF, 0) | rd.TU_SPLIT
        cbf = (t["cbf"].astype(np.int64) << np.arange(4)).sum(axis=-1)
        for m, (i, k, _, _, modes) in enumerate(items):
            out[i, k] = (int(dist[m]), int(cost[m]), int(bits[m]), int(flags[m]), int(cbf[m]), tuple(modes))
        if details is not None:
            details.update(D=t["D"], r=t["r"], where=[(it[0], it[1]) for it in items])
    return out


def as_record(nxn):
    """the NxN candidates as the records the stage writes where it takes them"""
    out = np.zeros(nxn.shape, PDT)
    out["dist"], out["cost_rd"], out["bits"], out["flags"] = nxn["dist"], nxn["cost_rd"], nxn["bits"], nxn["flags"]
    out["tu_split"], out["part"] = 1, PART_NXN
    return out


LESS, EQUAL, MORE, ALONE, INVALID = 0, 1, 2, 3, 4


def choose(two, nxn, outcome=None):
    """two: the 2Nx2N records [..., 64] MOTION_RD_PU_DTYPE, nxn [..., 64] INTRA_RD_NXN_DTYPE -> the stage's intra record per 8x8 node: NxN iff it is valid and
    strictly cheaper, or 2Nx2N is invalid (HM tries 2Nx2N first; xCheckBestMode keeps the earlier mode on a tie).  outcome: takes LESS / EQUAL / MORE (both
    valid), ALONE (NxN valid, 2Nx2N not), INVALID (no NxN)"""
    nv, tv = nxn["cost_rd"] != MARK, two["part"] != 255
    a, b = nxn["cost_rd"].astype(np.int64), two["cost_rd"].astype(np.int64)
    take = nv & (~tv | (a < b))
    if outcome is not None:
        outcome[...] = np.where(~nv, INVALID, np.where(~tv, ALONE, np.where(a < b, LESS, np.where(a == b, EQUAL, MORE))))
    return np.where(take, as_record(nxn), two)


def plain(pic, bd, qp, first, first4, rows=None, outcome=None, details=None):
    """-> (the intra records before gate and fold [band CTUs, 85], the NxN candidates [band CTUs, 64] or None); first4 None: intra_rd_qt_ref.plain at 3"""
    P = pic if isinstance(pic, ir.Picture) else ir.Picture(pic, bd)
    p = qt.plain(P, bd, qp, first, 3, rows)
    if first4 is None:
        return p, None
    x = candidates(P, bd, qp, first4, rows, details)
    p[:, NODE0:] = choose(p[:, NODE0:], x, outcome)
    return p, x


def expected(pic, bd, qp, first, first4, fold=None, rd_merge=None, skip_mask=0, rows=None, outcome=None):
    """one picture -> ([band CTUs, 85] MOTION_RD_PU_DTYPE, [band CTUs, 64] INTRA_RD_NXN_DTYPE or None); fold / rd_merge compact over the same rows, or None"""
    p, x = plain(pic, bd, qp, first, first4, rows, outcome)
    return ir.gate_fold(p, None if fold is None else fold.reshape(p.shape), None if rd_merge is None else rd_merge.reshape(p.shape), skip_mask), x


def same(got, exp, what=""):
    """every byte of every record, of either dtype"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    for f in got.dtype.names:
        bad = got[f] != exp[f]
        if bad.ndim > got.ndim:
            bad = bad.any(axis=-1)
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())


# ---- the draw: intra_rd_ref's 35 pictures with a first4 per picture ------------------------------------------------------------------------------------------

def real_first4(pic, bd, qp):
    """the oracle's 4x4 first pass of a picture, best records -> [numCtus, 256] NODE_DTYPE"""
    lib, _ = ir.oracle()
    H, W = pic.shape
    flat = np.ascontiguousarray(np.asarray(pic).astype(np.int16)).reshape(-1)
    return fp4.expected(lib, flat, 0, W, W, H, bd, qp)["best"]


def draw_first4(pic, bd, qp, seed, real):
    """real: the oracle's 4x4 records with their high mode bytes filled where the PU is valid; otherwise random bytes with modes uniform over 0..34 (four in
    ten: one of 0, 1, 10, 26), one record in twelve beyond 34 and one in twelve with the marker satd, as intra_rd_ref.draw_first draws"""
    rng = np.random.default_rng(9000 + seed)
    if real:
        a = real_first4(pic, bd, qp)
        inside = a["satd"] != MARK
        a["mode"] = np.where(inside, a["mode"] | (rng.integers(0, 1 << 24, size=a.shape) << 8).astype(np.uint32), a["mode"])
        return a
    shape = (ir.DRAW_N, 256)
    a = np.frombuffer(rng.bytes(shape[0] * shape[1] * 16), NDT).reshape(shape).copy()
    kind = rng.random(shape)
    special = rng.choice([0, 1, 10, 26], size=shape)
    mode = np.where(kind < 1 / 12, rng.integers(35, 256, size=shape), np.where(rng.random(shape) < 0.4, special, rng.integers(0, 35, size=shape)))
    a["mode"] = (a["mode"] & 0xFFFFFF00) | mode.astype(np.uint32)
    a["satd"] = np.where((kind >= 1 / 12) & (kind < 2 / 12), MARK, a["satd"] % 1000000)
    return a


def own_first4(first):
    """a first4 that repeats every 8x8 node's own mode (and satd) four times: first [n, 85] -> [n, 256]"""
    n = first.shape[0]
    a = np.zeros((n, 256), NDT)
    for k in range(NODES8):
        a[:, units(k)] = first[:, NODE0 + k][:, None]
    return a


@functools.lru_cache(maxsize=None)
def draw(index):
    """entry `index` of intra_rd_ref's DRAW -> dict: bd, qp, pic, first, first4, plain, nxn, outcome [n, 64], fold, merge (intra_rd_ref's records)"""
    d = ir.draw(index)
    _, _, seed, real = ir.DRAW[index]
    first4 = draw_first4(d["pic"], d["bd"], d["qp"], seed, real)
    outcome = np.zeros((ir.DRAW_N, NODES8), np.int64)
    p = qt.draw(index)["plain"].copy()   # the 2Nx2N records at three depths, shared with intra_rd_qt_ref's own tests
    x = candidates(d["pic"], d["bd"], d["qp"], first4)
    p[:, NODE0:] = choose(p[:, NODE0:], x, outcome)
    return dict(bd=d["bd"], qp=d["qp"], pic=d["pic"], first=d["first"], first4=first4, plain=p, nxn=x, outcome=outcome, fold=d["fold"], merge=d["merge"])


# ---- closed-form pictures ------------------------------------------------------------------------------------------------------------------------------------

STRIPE_MODES = (10, 26, 10, 26)


def quadrant_stripes(W, H, bd, x0, y0):
    """a constant picture whose 8x8 block at (x0, y0) (x0, y0 >= 1) has horizontal stripes in its left quadrants and vertical stripes in its right ones, every
    quadrant continuing the samples of its own line: modes STRIPE_MODES predict the four 4x4 blocks exactly.  The stripes are 0 / maximum by turns and
    start with the maximum, and the corner samples are 0: the edge filter of the pure directions only ever adds to a first row (column) that already holds
    the maximum, and the clip takes it back"""
    hi = (1 << bd) - 1
    pic = qt.constant_picture(W, H, bd)
    rows = np.array([hi, 0] * 4)   # the column left of the block: quadrants 0 and 2 repeat it along x
    cols = np.array([hi, 0] * 2)   # the row above quadrant 1: quadrants 1 and 3 repeat it along y
    pic[y0 - 1, x0 - 1:x0 + 4] = 0            # the corner of quadrant 0 and the row above it, whose last sample is quadrant 1's corner
    pic[y0:y0 + 8, x0 - 1] = rows
    pic[y0 - 1, x0 + 4:x0 + 8] = cols
    pic[y0:y0 + 8, x0:x0 + 4] = rows[:, None]
    pic[y0:y0 + 8, x0 + 4:x0 + 8] = cols[None, :]
    return pic
