"""Expected values of the RD stages with the depth count as an argument (fhevc_motion_rd_qt*, fhevc_motion_rd_pu_qt*, fhevc_p_tree_rd_qt_frame), restated
in numpy from the definition in include/fasthevc.h -- not from the C code.  Per TU everything is motion_rd_ref.tu_pass (pinned to the reference's own
transforms and quantiser by tests/test_motion_rd_ref.py); what is new here is HM's nested choice over three TU depths as a pure function of per-TU
(D, r, cbf) arrays, of which two depths are the special case.  The PU form reuses motion_rd_pu_ref's vector choice, composed prediction and fold.
tests/test_motion_rd_qt_ref.py holds this module against the two-depth modules and against hand-set numbers without a GPU.  A plain module, not a
conftest and not a test."""
import numpy as np

import motion_rd_pu_ref as pu
import motion_rd_ref as rd
import motion_refine_ref as mr

MARK, SAT = rd.MARK, rd.SAT
TU_SIZES = {2: rd.TU_SIZES, 3: {64: (32, 16), 32: (32, 16, 8), 16: (16, 8, 4), 8: (8, 4)}}   # node side -> the TU sizes per depth


def nested_choice(D0, r0, cbf0, D1, r1, cbf1, D2, r2, cbf2, lam, third=True):
    """one depth-0 TU: D0, r0, cbf0 [...]; its four depth-1 TUs [..., 4]; their four children each [..., 4, 4] (ignored unless `third`) -> dict of
    J (the chosen cost without side bits), dist, rate (everything lam multiplies in J), take0 [...], take1 [..., 4], coded [..., 4], K1, K2, J0, J1"""
    D0, r0, D1, r1 = (np.asarray(a, np.int64) for a in (D0, r0, D1, r1))
    cbf1 = np.asarray(cbf1, bool)
    if third:
        D2s, r2s, any2 = np.asarray(D2, np.int64).sum(axis=-1), np.asarray(r2, np.int64).sum(axis=-1), np.asarray(cbf2, bool).any(axis=-1)
        K1 = 256 * D1 + lam * (1 + r1)                    # with this TU's own split flag
        K2 = 256 * D2s + lam * (1 + r2s)
        take1 = any2 & (K2 < K1)
    else:
        D2s, r2s = np.zeros_like(D1), np.zeros_like(r1)
        K1 = 256 * D1 + lam * r1                          # no flag: it cannot split
        K2 = np.zeros_like(K1)
        take1 = np.zeros(K1.shape, bool)
    C = np.where(take1, K2, K1)
    coded = take1 | cbf1
    J0 = 256 * D0 + lam * (1 + r0)
    J1 = C.sum(axis=-1) + lam
    take0 = coded.any(axis=-1) & (J1 < J0)
    own = (1 if third else 0) + np.where(take1, r2s, r1)   # what lam multiplies in C
    return dict(J=np.where(take0, J1, J0), dist=np.where(take0, np.where(take1, D2s, D1).sum(axis=-1), D0), rate=np.where(take0, 1 + own.sum(axis=-1), 1 + r0),
                take0=take0, take1=take1 & take0[..., None], would1=take1, coded=coded, K1=K1, K2=K2, J0=J0, J1=J1)


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


def node_records(org, pred, bd, qp, side, tu_depths=3, detail=None):
    """org, pred: [M, s, s] nodes of one size, side: [M] side bits -> (dist, cost_rd, bits, flags, tu_split) arrays [M]"""
    assert tu_depths in (2, 3)
    s = org.shape[-1]
    sizes = TU_SIZES[tu_depths][s]
    lam = rd.lam_q8(qp)
    o0, p0 = rd.split(np.asarray(org, np.int64), sizes[0]), rd.split(np.asarray(pred, np.int64), sizes[0])     # [M, T, n0, n0]
    o1, p1 = rd.split(o0, sizes[1]), rd.split(p0, sizes[1])                                                     # [M, T, 4, n1, n1]
    a, b = rd.tu_pass(o0, p0, bd, qp), rd.tu_pass(o1, p1, bd, qp)
    third = len(sizes) == 3
    c = rd.tu_pass(rd.split(o1, sizes[2]), rd.split(p1, sizes[2]), bd, qp) if third else dict(D=None, r=None, cbf=None)   # [M, T, 4, 4, n2, n2]
    ch = nested_choice(a["D"], a["r"], a["cbf"], b["D"], b["r"], b["cbf"], c["D"], c["r"], c["cbf"], lam, third)
    if detail is not None:
        detail.update(ch, cbf0=a["cbf"], cbf1=b["cbf"], third=third)
    return node_from_choice(ch, a["cbf"], a["zero_half"], side, lam)


def expected(cur, ref_pic, W, H, bd, qp, records, source, max_range, tu_depths=3, mvp=None, rows=None, planes=None, details=None):
    """motion_rd_ref.expected with the depth count; details: a dict that takes, per level, the nested choice's arrays"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    records = records.reshape(nb, 85)
    assert source in (rd.MERGE, rd.EXPLICIT) and (mvp is None or source == rd.EXPLICIT)
    mvp = mvp.reshape(nb, 85) if mvp is not None else None
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    assert planes.pad >= max_range + 6 and planes.bd == bd
    cur = np.asarray(cur, np.int64)
    reach = 4 * max_range + 3
    out = np.zeros((nb, 85), rd.RDT)
    out[:] = rd.INVALID
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
            if source == rd.MERGE:
                side = int(rd.merge_side_bits(rec["idx"]))
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
        detail = {} if details is not None else None
        dist, cost, bits, flags, tus = node_records(np.stack([t[2] for t in items]), np.stack([t[3] for t in items]), bd, qp, [t[4] for t in items], tu_depths, detail)
        for m, (i, k, _, _, _, q) in enumerate(items):
            out[i, k] = (int(dist[m]), int(cost[m]), int(bits[m]), int(flags[m]), int(tus[m]), q[0], q[1])
        if details is not None:
            details[lvl] = detail
    return out


def expected_pu(cur, ref_pic, W, H, bd, qp, part_mode, inp, max_range, tu_depths=3, rows=None, planes=None, fold_into=None):
    """motion_rd_pu_ref.expected with the depth count: its vector choice, its composed prediction, its fold"""
    assert part_mode in pu.MODES
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    assert planes.pad >= max_range + 6 and planes.bd == bd
    cur = np.asarray(cur, np.int64)
    reach = 4 * max_range + 3
    out = pu.marker((nb, 85))
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
            p = pu.size_of(part_mode, inp.shapes[i, k] if part_mode >= pu.BEST else None)
            got = pu.node_choice(inp, i, k, p, reach)
            if got is None:
                continue
            shape, vecs, side, merged = got
            todo[lvl].append((i, k, cur[y0:y0 + n, x0:x0 + n], pu.composed(planes, k, shape, vecs, x0, y0, n), side, p, merged))
    for lvl, items in todo.items():
        if not items:
            continue
        dist, cost, bits, flags, tus = node_records(np.stack([t[2] for t in items]), np.stack([t[3] for t in items]), bd, qp, [t[4] for t in items], tu_depths)
        for m, (i, k, _, _, _, p, merged) in enumerate(items):
            out[i, k] = (int(dist[m]), int(cost[m]), int(bits[m]), int(flags[m]), int(tus[m]), p, merged, (0, 0))
    return out if fold_into is None else pu.fold(out, fold_into.reshape(nb, 85))


def frame_records(cur, ref_pic, Wp, Hp, bd, qp, max_range, inp, merge_nodes, skip_mask, tu_depths=3, rule=None, planes=None):
    """motion_rd_pu_ref.frame_records with all four RD launches at tu_depths -> (rd_merge, rd_pu, depth_min, depth_max)"""
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    rd_merge = expected(cur, ref_pic, Wp, Hp, bd, qp, merge_nodes, rd.MERGE, max_range, tu_depths, planes=planes)
    acc = expected_pu(cur, ref_pic, Wp, Hp, bd, qp, 0, inp, max_range, tu_depths, planes=planes)
    for mode in (pu.BEST, pu.SECOND):
        acc = expected_pu(cur, ref_pic, Wp, Hp, bd, qp, mode, inp, max_range, tu_depths, planes=planes, fold_into=acc)
    _, dmin, dmax = rd.tree_select(acc[None], rd_merge[None], skip_mask, Wp, Hp, rule=rule)
    return rd_merge, acc, dmin[0], dmax[0]


# ---- a node whose residual is confined to one N2 block: the constructed cases of the tests -----------------------------------------------------------------

def confined_node(s, i, sub, bd=8, amp=60):
    """(org, pred) [s, s] of a node of side s = 32 or 16: a flat prediction, and an original that differs from it by a checkerboard of +-amp inside ONE block
    of side s / 4 -- child `sub` (raster) of depth-1 TU i (raster)"""
    n1, n2 = s // 2, s // 4
    mid = 1 << (bd - 1)
    pred = np.full((s, s), mid, np.int64)
    org = pred.copy()
    y0, x0 = (i >> 1) * n1 + (sub >> 1) * n2, (i & 1) * n1 + (sub & 1) * n2
    yy, xx = np.mgrid[0:n2, 0:n2]
    org[y0:y0 + n2, x0:x0 + n2] += np.where((xx + yy) % 2 == 0, amp, -amp)
    return org, pred


# A node where the FIRST condition of take1 decides.  With exact transforms it cannot: a coded depth-1 TU always gains more distortion than its levels cost.
# At 12 bit xGetSSE's per-sample shift (>> 8) drops every error below 16, so a faint pattern has D = 0 coded or not, and a depth-1 TU that codes two levels
# of it (r1 = 6 at QP 8) is dearer than its four children, which code nothing (K2 = 5 lam < K1 = 7 lam) -- and still must not split.  A strong checkerboard in
# another depth-1 TU makes the depth-0 TU split, so the record shows which way depth 1 went.
UNPAID_BD, UNPAID_QP = 12, 8
UNPAID_PATTERN = np.array([[-3, 7, -7, 3, 3, -7, 7, -3], [5, -12, 12, -5, -5, 12, -12, 5], [-1, 2, -2, 1, 1, -2, 2, -1], [-4, 10, -10, 4, 4, -10, 10, -4],
                           [4, -10, 10, -4, -4, 10, -10, 4], [1, -2, 2, -1, -1, 2, -2, 1], [-5, 12, -12, 5, 5, -12, 12, -5], [3, -7, 7, -3, -3, 7, -7, 3]], np.int64)


def unpaid_node(amp=40):
    """(org, pred) [16, 16] at UNPAID_BD bits: the faint pattern in depth-1 TU 1, a checkerboard of +-amp in depth-1 TU 2"""
    pred = np.full((16, 16), 1 << (UNPAID_BD - 1), np.int64)
    org = pred.copy()
    org[0:8, 8:16] += UNPAID_PATTERN
    yy, xx = np.mgrid[0:8, 0:8]
    org[8:16, 0:8] += np.where((xx + yy) % 2 == 0, amp, -amp)
    return org, pred


# ---- the draw: motion_rd_ref's 168 x 152 pictures with content that only the smallest transform sees ---------------------------------------------------------
# motion_rd_ref's own draw shows no depth-0 TU that is coded at depth 2 alone and too few 32x32 nodes that get dearer, so the flat corner of its current
# picture is redrawn here: per 32x32 block one amplitude a (some step of the draw's QPs lies in [a / 0.208, a / 0.104) for most of them); one of its 16x16
# quarters holds an aligned 8x8 bump of +-a -- its DC is 8 a at N = 8 and 4 a at N = 16 --, the other three an aligned 4x4 bump of +-2 a -- 8 a at N = 4,
# 4 a at N = 8.  The reference stays flat there, so every vector of the draw that stays in the corner predicts the flat value.  Three draws of records.

DRAW_RECORD_SEEDS = (5, 6, 7)
DRAW_AMPS = (1, 2, 3, 5, 7, 12, 24, 32, 40)


def draw_pictures(bd, seed=0):
    """(reference, current) [152, 168] int64: motion_rd_ref.draw_pictures with the bumps in the flat corner of the current picture"""
    ref, cur = rd.draw_pictures(bd, seed)
    rng = np.random.default_rng(77 + bd)
    cur[64:, 64:] = ((1 << bd) - 1) // 3
    for by in range(64, rd.DRAW_H - 31, 32):
        for bx in range(64, rd.DRAW_W - 31, 32):
            a = int(rng.choice(DRAW_AMPS)) << (bd - 8)
            q8 = int(rng.integers(0, 4))
            for qd in range(4):
                y0, x0 = by + (qd >> 1) * 16, bx + (qd & 1) * 16
                sgn = int(rng.choice([-1, 1]))
                if qd == q8:
                    oy, ox = 8 * int(rng.integers(0, 2)), 8 * int(rng.integers(0, 2))
                    cur[y0 + oy:y0 + oy + 8, x0 + ox:x0 + ox + 8] += sgn * a
                else:
                    oy, ox = 4 * int(rng.integers(0, 4)), 4 * int(rng.integers(0, 4))
                    cur[y0 + oy:y0 + oy + 4, x0 + ox:x0 + ox + 4] += sgn * 2 * a
    return ref, cur
