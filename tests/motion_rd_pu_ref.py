"""Expected values of the RD stage under a partition size (fhevc_motion_rd_pu*), of its fold and of the frame call that chains them
(fhevc_p_tree_rd_frame), restated in numpy from the definitions in include/fasthevc.h -- not from the C code -- on top of motion_rd_ref.node_records:
the composed prediction is planes.block at each part's vector, chosen per sample by the rectangle motion_pu_ref.pu_rect gives (getPartIndexAndSize),
the parts come from pu_shape_ref.parts, the merged rule is the selection's (merge cost strictly below the refined cost).  A numpy model of the KERNEL's
quadrant arithmetic lives here too, only so that tests/test_motion_rd_pu_ref.py can hold it against pu_rect.  A plain module, not a conftest and not a test."""
from collections import namedtuple

import numpy as np

import motion_merge_pu_ref as mgp
import motion_pu_ref as mp
import motion_rd_ref as rd
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
import pu_shape_ref as sr
from fasthevc_amd import capi

MARK, SAT = rd.MARK, rd.SAT
RPT = capi.MOTION_RD_PU_DTYPE
QDT, MDT, PDT, SDT = capi.MOTION_QPEL_DTYPE, capi.MOTION_MERGE_DTYPE, capi.MOTION_MVP_DTYPE, capi.SHAPE_DTYPE
INVALID = (MARK, MARK, 0xFFFF, 0, 0, 255, 0, (0, 0))
FORCED = (0, 1, 2, 4, 5, 6, 7)
BEST, SECOND = capi.RD_PART_BEST, capi.RD_PART_SECOND
MODES = FORCED + (BEST, SECOND)
TWO_PART = (1, 2, 4, 5, 6, 7)

# the arrays of fhevc_motion_rd_pu_inputs but fold: [band CTUs, 85 / 124 / 384] each, or None
Inputs = namedtuple("Inputs", "nodes pus pus_small merge_pus merge_pus_small mvp_nodes mvp_pus mvp_pus_small shapes", defaults=(None,) * 8)


def marker(shape):
    out = np.zeros(shape, RPT)
    out[...] = INVALID
    return out


def size_of(part_mode, shape_rec):
    """the PartSize the launch prices for a node: forced, or a byte of its selection record"""
    if part_mode == BEST:
        return int(shape_rec["best"])
    if part_mode == SECOND:
        return int(shape_rec["second"])
    return part_mode


def part_choice(refined, merge, mvp, reach):
    """one part: its refined record, its merge record or None, its predictor record or None -> (valid, (mvx, mvy), side bits, merged)"""
    rc = int(refined["cost_best"])
    mc = int(merge["cost_best"]) if merge is not None else MARK
    merged = mc < rc                                          # strictly: a marker loses to anything
    if merged:
        q, side, ok = (int(merge["mvx"]), int(merge["mvy"])), int(rd.merge_side_bits(int(merge["idx"]))), True
    else:
        q, ok = (int(refined["mvx"]), int(refined["mvy"])), rc != MARK    # both markers: invalid
        if mvp is not None:
            ok, side = ok and int(mvp["idx"]) != 255, int(mvp["bits"])
        else:
            side = mr.eg_bits(q[0]) + mr.eg_bits(q[1])
    return ok and abs(q[0]) <= reach and abs(q[1]) <= reach, q, side, merged


def node_choice(inp, i, k, p, reach):
    """node k of CTU i of the band under size p -> None (unavailable or a part invalid) or (shape or None for 2Nx2N, [vector per part], side bits, merged)"""
    if p == 0:
        ok, q, side, _ = part_choice(inp.nodes[i, k], None, None if inp.mvp_nodes is None else inp.mvp_nodes[i, k], reach)
        return (None, [q], side, 0) if ok else None
    where = sr.parts(k, p) if p in TWO_PART else None
    if where is None:
        return None
    fam, merge, mvp = (inp.pus, inp.merge_pus, inp.mvp_pus) if where[0] == "pu" else (inp.pus_small, inp.merge_pus_small, inp.mvp_pus_small)
    if fam is None:
        return None
    got = [part_choice(fam[i, e], None if merge is None else merge[i, e], None if mvp is None else mvp[i, e], reach) for e in where[1:]]
    if not (got[0][0] and got[1][0]):
        return None
    return sr.shape_of(p), [got[0][1], got[1][1]], got[0][2] + got[1][2], (1 if got[0][3] else 0) | (2 if got[1][3] else 0)


def composed(planes, k, shape, vecs, x0, y0, n):
    """the prediction of node k (n x n at picture position (x0, y0)): per part the block at that part's vector, inside that part's rectangle"""
    if shape is None:
        return planes.block(vecs[0][0], vecs[0][1], x0, y0, n).astype(np.int64)
    nx, ny, _ = mp.node_rect(k)
    pred = np.zeros((n, n), np.int64)
    for part in (0, 1):
        px, py, w, h = mp.pu_rect(k, shape, part)
        blk = planes.block(vecs[part][0], vecs[part][1], x0, y0, n)
        pred[py - ny:py - ny + h, px - nx:px - nx + w] = blk[py - ny:py - ny + h, px - nx:px - nx + w]
    return pred


def fold(new, old):
    """the record written: the new one iff it is valid and (the earlier one is a marker or the new cost_rd is strictly smaller); else the earlier bytes"""
    take = (new["cost_rd"] != MARK) & (new["cost_rd"] < old["cost_rd"])      # a marker's cost_rd is the largest number
    out = old.copy()
    out[take] = new[take]
    return out


def fold_outcome(new, old):
    """per record: 0 new wins, 1 earlier wins, 2 tie, 3 earlier is a marker (new valid), 4 new is a marker"""
    n, o = new["cost_rd"].astype(np.int64), old["cost_rd"].astype(np.int64)
    return np.where(n == MARK, 4, np.where(o == MARK, 3, np.where(n < o, 0, np.where(n == o, 2, 1))))


def expected(cur, ref_pic, W, H, bd, qp, part_mode, inp, max_range, rows=None, planes=None, fold_into=None, seen=None):
    """cur / ref_pic: the samples [H, W]; inp: Inputs, compact over the CTU rows `rows`; fold_into: [band CTUs, 85] RPT or None -> [band CTUs, 85] RPT.
    seen: a dict that takes, per (level, p), the number of valid nodes whose two parts hold different vectors"""
    assert part_mode in MODES
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    assert planes.pad >= max_range + 6 and planes.bd == bd
    cur = np.asarray(cur, np.int64)
    reach = 4 * max_range + 3
    out = marker((nb, 85))
    todo = {l: [] for l in range(4)}
    for i in range(nb):
        c = rows[0] * cw + i
        cx, cy = c % cw, c // cw
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            n = 64 >> lvl
            x0, y0 = cx * 64 + bx * n, cy * 64 + by * n
            if x0 + n > W or y0 + n > H:
                continue
            p = size_of(part_mode, inp.shapes[i, k] if part_mode >= BEST else None)
            ch_ = node_choice(inp, i, k, p, reach)
            if ch_ is None:
                continue
            shape, vecs, side, merged = ch_
            if seen is not None and shape is not None and vecs[0] != vecs[1]:
                seen[(lvl, p)] = seen.get((lvl, p), 0) + 1
            todo[lvl].append((i, k, cur[y0:y0 + n, x0:x0 + n], composed(planes, k, shape, vecs, x0, y0, n), side, p, merged))
    for lvl, items in todo.items():
        if not items:
            continue
        dist, cost, bits, flags, tus = rd.node_records(np.stack([t[2] for t in items]), np.stack([t[3] for t in items]), bd, qp, [t[4] for t in items])
        for m, (i, k, _, _, _, p, merged) in enumerate(items):
            out[i, k] = (int(dist[m]), int(cost[m]), int(bits[m]), int(flags[m]), int(tus[m]), p, merged, (0, 0))
    return out if fold_into is None else fold(out, fold_into.reshape(nb, 85))


def same(got, exp, what=""):
    """every byte of every record"""
    assert got.shape == exp.shape and got.dtype == exp.dtype == RPT, (what, got.shape, exp.shape)
    for f in RPT.names:
        bad = got[f] != exp[f]
        if f == "pad":
            bad = bad.any(axis=-1)
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())


# ---- the kernel's quadrant -> part arithmetic, as numpy: lane = tile (tx, ty) of wave = level, quadrant q = 2 (row half) + (column half) ----------------------

def kernel_quadrant_part(lvl, tx, ty, p, q):
    """which part of size p of the tile's node at level lvl holds 4x4 quadrant q of tile (tx, ty): positions in 4-sample units against the cut"""
    tn, s4 = 8 >> lvl, 16 >> lvl
    horiz = p in (1, 4, 5)
    cut = s4 // 2 if p <= 2 else (3 * s4 // 4 if p & 1 else s4 // 4)
    at = ((ty & (tn - 1)) * 2 + (q >> 1)) if horiz else ((tx & (tn - 1)) * 2 + (q & 1))
    return 1 if at >= cut else 0


def straddles(lvl, tx, ty, p):
    return len({kernel_quadrant_part(lvl, tx, ty, p, q) for q in range(4)}) == 2


# ---- pictures built by the filter itself: two motions inside one CU, for sizes motion_refine_pu_ref has no kind for ---------------------------------------------

# kind -> (family, shape, the CU nodes it is about, first(xx, yy): the samples of part 0, coordinates inside the CTU), as rp.TWO_MOTION_KINDS
TWO_MOTION_KINDS = dict(rp.TWO_MOTION_KINDS)
TWO_MOTION_KINDS.update({
    "2NxnD@16": ("small", 3, range(5, 21), lambda xx, yy: yy % 16 < 12),
    "nRx2N@16": ("small", 5, range(5, 21), lambda xx, yy: xx % 16 < 12),
    "Nx2N@32": ("pu", 1, range(1, 5), lambda xx, yy: xx % 32 < 16),
    "2NxnU@32": ("pu", 2, range(1, 5), lambda xx, yy: yy % 32 < 8),
    "2NxN@64": ("pu", 0, range(0, 1), lambda xx, yy: yy % 64 < 32),
})
KIND_ORDER = ("2NxnU@16", "nLx2N@16", "2NxN@8", "Nx2N@8", "2NxN@32", "2NxnD@16", "nRx2N@16", "Nx2N@32", "2NxnU@32", "2NxN@64")


def part_size_of_kind(kind):
    shape = TWO_MOTION_KINDS[kind][1]
    return shape + 1 if shape <= 1 else shape + 2


def two_motion_picture(planes, kinds, qa, qb):
    """rp.two_motion_picture over TWO_MOTION_KINDS of this module: [64, 64 * len(kinds)], CTU i holds in part 0 of every CU of kinds[i] the reference
    displaced by qa (quarter samples), elsewhere by qb, samples taken from the fractional planes themselves"""
    H, W = 64, 64 * len(kinds)

    def displaced(q):
        a = planes.planes[q[1] & 3][q[0] & 3]
        y, x = planes.pad + (q[1] >> 2), planes.pad + (q[0] >> 2)
        return a[y:y + H, x:x + W].astype(np.int64)

    yy, xx = np.mgrid[0:H, 0:W]
    first = np.zeros((H, W), bool)
    for i, kind in enumerate(kinds):
        sel = slice(64 * i, 64 * i + 64)
        first[:, sel] = TWO_MOTION_KINDS[kind][3](xx[:, sel] % 64, yy[:, sel])
    return np.where(first, displaced(qa), displaced(qb))


def two_motion_inputs(kinds, qa, qb, cost=1000):
    """Inputs for two_motion_picture's CTUs: qa in every part 0, qb in every part 1 of both PU families, qa in the nodes; no merge, no predictor records"""
    n = len(kinds)
    nodes, pus, small = np.zeros((n, 85), QDT), np.zeros((n, 124), QDT), np.zeros((n, 384), QDT)
    for a, cov in ((pus, mp.covered()), (small, rp.FAMILIES["small"][0]())):
        part = np.array([p for _, _, p in cov])
        a["mvx"], a["mvy"] = np.where(part == 0, qa[0], qb[0]), np.where(part == 0, qa[1], qb[1])
    nodes["mvx"], nodes["mvy"] = qa
    for a in (nodes, pus, small):
        a["cost_best"] = cost
    return Inputs(nodes, pus, small)


# ---- the draw: the RD tests' 168 x 152 pictures, PU records within the reach, merge records a hair around them ------------------------------------------------

W, H, CW, CH, N = rd.DRAW_W, rd.DRAW_H, rd.DRAW_CW, rd.DRAW_CH, rd.DRAW_N
MAIN_SEED, MAIN_PAIRS = 4, 6      # the GPU test's main draw: six picture pairs, so that the level of the 64x64 nodes holds 24 of them


def draw_inputs(seed, max_range, nf=2, with_merge=True, with_mvp=True, with_small=True):
    """[nf - 1] Inputs of random bytes: refined records from motion_merge_pu_ref.random_refined (vectors of a pool inside the reach, one in ten beyond it, one
    in seven marked), merge records in the manner of random_pu_merge (cost a hair around the refined one, equal, or the marker) with vectors of their own,
    predictor records with one marker in ten, selection records whose best / second are any of the seven sizes, 3 or 255"""
    rng = np.random.default_rng(seed)
    reach = 4 * max_range + 3
    pool = [(-5, 2), (3, 3), (reach, -reach), (0, -7), (6, 4), (-reach, 9), (1, reach), (7, 5)]
    out = []
    for _ in range(nf - 1):
        nodes, pus, small = (mgp.random_refined(rng, (N, per), max_range, pool=pool) for per in (85, 124, 384))
        merges = mgp.random_pu_merge(rng, pus, small)
        for m in merges:
            pick = np.array(pool, np.int16)[rng.integers(0, len(pool), size=m.shape)]
            far = rng.random(m.shape) < 0.05
            m["mvx"], m["mvy"] = np.where(far, reach + 1, pick[..., 0]), pick[..., 1]
            m["idx"] = np.where(rng.random(m.shape) < 0.05, rng.integers(5, 256, size=m.shape), rng.integers(0, 5, size=m.shape))
        mvps = []
        for per in (85, 124, 384):
            v = np.frombuffer(rng.bytes(N * per * 8), PDT).reshape(N, per).copy()
            v["idx"] = np.where(rng.random(v.shape) < 0.1, 255, rng.integers(0, 2, size=v.shape))
            v["bits"] = rng.integers(2, 67, size=v.shape)
            mvps.append(v)
        shapes = np.frombuffer(rng.bytes(N * 85 * 16), SDT).reshape(N, 85).copy()
        choice = np.array([0, 1, 2, 4, 5, 6, 7, 1, 2, 4, 5, 6, 7, 3, 255], np.uint8)
        shapes["best"], shapes["second"] = choice[rng.integers(0, len(choice), size=(N, 85))], choice[rng.integers(0, len(choice), size=(N, 85))]
        out.append(Inputs(nodes, pus, small if with_small else None, merges[0] if with_merge else None, merges[1] if with_merge and with_small else None,
                          mvps[0] if with_mvp else None, mvps[1] if with_mvp else None, mvps[2] if with_mvp and with_small else None, shapes))
    return out


def band_of(inp, rows):
    """the Inputs of a band of CTU rows: exact slices"""
    return Inputs(*[None if a is None else np.ascontiguousarray(a[rows[0] * CW:rows[1] * CW]) for a in inp])


def draw_statistics(inp, max_range):
    """what a draw holds on INSIDE nodes -> dict: merged[lvl] = [nodes with a merged part, without], straddling[lvl] = tiles that straddle a cut of a valid node"""
    reach = 4 * max_range + 3
    merged, straddling = {l: [0, 0] for l in range(4)}, {l: 0 for l in range(4)}
    for i in range(N):
        cx, cy = i % CW, i // CW
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            n = 64 >> lvl
            if cx * 64 + (bx + 1) * n > W or cy * 64 + (by + 1) * n > H:
                continue
            for p in TWO_PART:
                got = node_choice(inp, i, k, p, reach)
                if got is None:
                    continue
                merged[lvl][0 if got[3] else 1] += 1
                if got[1][0] != got[1][1]:
                    t = n // 8
                    straddling[lvl] += sum(straddles(lvl, bx * t + x, by * t + y, p) for y in range(max(t, 1)) for x in range(max(t, 1)))
    return dict(merged=merged, straddling=straddling)


# ---- the frame call: fhevc_p_tree_rd_frame from the records its chain made -----------------------------------------------------------------------------------

def frame_records(cur, ref_pic, Wp, Hp, bd, qp, max_range, inp, merge_nodes, skip_mask, rule=None, planes=None):
    """the chain behind the selection, from the selection's inputs `inp` (re-priced entries, PU merge records, predictor records, shapes) and the nodes' merge
    records: the RD records of the merge records, the three folded launches (2Nx2N, best, second), the RD tree -> (rd_merge, rd_pu, depth_min, depth_max)"""
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    rd_merge = rd.expected(cur, ref_pic, Wp, Hp, bd, qp, merge_nodes, rd.MERGE, max_range, planes=planes)
    acc = expected(cur, ref_pic, Wp, Hp, bd, qp, 0, inp, max_range, planes=planes)
    for mode in (BEST, SECOND):
        acc = expected(cur, ref_pic, Wp, Hp, bd, qp, mode, inp, max_range, planes=planes, fold_into=acc)
    _, dmin, dmax = rd.tree_select(acc[None], rd_merge[None], skip_mask, Wp, Hp, rule=rule)
    return rd_merge, acc, dmin[0], dmax[0]
