"""Expected values of the intra RD stage that searches the first pass's candidate lists (fhevc_intra_rd_search*, fhevc_p_tree_rd_intra_search_frame), restated
in numpy from the definition in include/fasthevc.h -- not from the C code.  Composed from intra_rd_qt_ref (the record F(m) of every node at a mode and, from
its details, J0 per depth-0 TU: A_c) and intra_rd_nxn_ref (the NxN record, the choice against 2Nx2N, gate and fold); the 4x4 PUs are priced one by one with
intra_rd_qt_ref.tu_pass.  tests/test_intra_rd_search_ref.py holds this module to closed forms without a GPU; tests/test_gpu_intra_rd_search.py compares the
library with it.  A plain module, not a conftest and not a test."""
import functools

import numpy as np

import intra_rd_nxn_ref as nx
import intra_rd_qt_ref as qt
import intra_rd_ref as ir
import motion_rd_ref as rd
from fasthevc_amd import capi

MARK, SAT = rd.MARK, rd.SAT
PDT, NDT, XDT = capi.MOTION_RD_PU_DTYPE, capi.NODE_DTYPE, capi.INTRA_RD_NXN_DTYPE
DEFAULT = dict(count=(3, 3, 3, 8), count4=8, append_planar=1)
LEVEL = np.array([0] + [1] * 4 + [2] * 16 + [3] * 64)


def rule_of(rule):
    """a dict like DEFAULT -> capi.IntraSearchRule"""
    return capi.intra_search_rule(rule["count"], rule["count4"], rule["append_planar"])


def candidates_of(entry, count, append_planar):
    """the bytes of one list entry -> [(position, mode)]: the first `count` bytes in order, bytes > 34 skipped; with append_planar mode 0 behind them, at
    position `count`, iff there is a valid entry and none of them is 0"""
    out = [(p, int(b)) for p, b in enumerate(entry[:count]) if int(b) <= 34]
    if append_planar and out and all(m != 0 for _, m in out):
        out.append((count, 0))
    return out


def best_second(costs):
    """HM's bookkeeping over step A's costs in list order -> (index of the best or None, index of the second or None): strictly below the best becomes the best
    and the old best the second; otherwise strictly below the second becomes the second"""
    best = second = None
    for i, a in enumerate(costs):
        if best is None or a < costs[best]:
            best, second = i, best
        elif second is None or a < costs[second]:
            second = i
    return best, second


_MODES = {}


def _per_mode(P, bd, qp, nb, rows):
    """F(m), its unshifted J and A(m) of every node of the band, mode by mode, computed when first asked for and kept per picture, depth, QP and band: the
    rules and lists a picture is priced under share them"""
    lam = rd.lam_q8(qp)
    cache = _MODES.setdefault((hash(P.pic.tobytes()), P.pic.shape, bd, qp, tuple(rows)), {})

    def at(m):
        if m not in cache:
            first = np.zeros((nb, 85), NDT)
            first["mode"] = m
            details = {}
            rec = qt.plain(P, bd, qp, first, 3, rows, details)
            J = np.zeros((nb, 85), np.int64)
            A = np.zeros((nb, 85), np.int64)
            side = ir.mode_bits(m)
            for lvl, d in details.items():
                for n, (i, k) in enumerate(d["where"]):
                    J[i, k] = int(d["J"][n].sum()) + lam * side
                    A[i, k] = int(d["J0"][n].sum()) + lam * side
            cache[m] = (rec, J, A)
        return cache[m]
    return at


def pu_choice(P, bd, qp, modes4, rule, rows, nb, cw):
    """per 4x4 PU the candidate with the smallest 256 D + lam (r + bits(m)), strict < in list order -> dict of [nb, 256] arrays: mode (255: none), D, r, cbf,
    zero_half"""
    lam = rd.lam_q8(qp)
    out = dict(mode=np.full((nb, 256), 255, np.int64), D=np.zeros((nb, 256), np.int64), r=np.zeros((nb, 256), np.int64), cbf=np.zeros((nb, 256), bool),
               zero_half=np.zeros((nb, 256), bool))
    items = []
    for i in range(nb):
        c = rows[0] * cw + i
        cx, cy = c % cw, c // cw
        for u in range(256):
            x0, y0 = cx * 64 + (u % 16) * 4, cy * 64 + (u // 16) * 4
            if x0 + 4 > P.W or y0 + 4 > P.H:
                continue
            for _, m in candidates_of(modes4[i, u], rule["count4"], rule["append_planar"]):
                items.append((i, u, m, P.pic[y0:y0 + 4, x0:x0 + 4], P.predict(x0, y0, 4, m)))
    if not items:
        return out
    t = qt.tu_pass(np.stack([it[3] for it in items]), np.stack([it[4] for it in items]), bd, qp)
    best = {}
    for n, (i, u, m, _, _) in enumerate(items):
        j = 256 * int(t["D"][n]) + lam * (int(t["r"][n]) + ir.mode_bits(m))
        if (i, u) not in best or j < best[(i, u)][0]:
            best[(i, u)] = (j, n, m)
    for (i, u), (_, n, m) in best.items():
        out["mode"][i, u], out["D"][i, u], out["r"][i, u] = m, int(t["D"][n]), int(t["r"][n])
        out["cbf"][i, u], out["zero_half"][i, u] = bool(t["cbf"][n]), bool(t["zero_half"][n])
    return out


def nxn_records(P, pu, rows, nb, cw, qp):
    """the NxN candidates over the four chosen modes [nb, 64] INTRA_RD_NXN_DTYPE: valid iff the node is inside and every PU has a mode"""
    lam = rd.lam_q8(qp)
    out = np.zeros((nb, nx.NODES8), XDT)
    out[:] = nx.NXN_MARKER
    for i in range(nb):
        c = rows[0] * cw + i
        cx, cy = c % cw, c // cw
        for k in range(nx.NODES8):
            x0, y0 = cx * 64 + (k % 8) * 8, cy * 64 + (k // 8) * 8
            us = nx.units(k)
            modes = [int(pu["mode"][i, u]) for u in us]
            if x0 + 8 > P.W or y0 + 8 > P.H or any(m > 34 for m in modes):
                continue
            D, r = pu["D"][i, us], pu["r"][i, us]
            dist, cost, bits = nx.nxn_cost(D, r, sum(ir.mode_bits(m) for m in modes), lam)
            flags = (0 if pu["cbf"][i, us].any() else rd.ZERO_PLAIN) | (rd.ZERO_HALF if pu["zero_half"][i, us].all() else 0) | rd.TU_SPLIT
            cbf = sum(int(pu["cbf"][i, u]) << j for j, u in enumerate(us))
            out[i, k] = (int(dist), int(cost), int(bits), int(flags), cbf, tuple(modes))
    return out


def plain(pic, bd, qp, modes, modes4, rule=None, rows=None, stats=None):
    """pic [H, W] (or an intra_rd_ref.Picture); modes [band CTUs, 85, stride] uint8, modes4 [band CTUs, 256, stride4] uint8 or None -> (the intra records before
    gate and fold [band CTUs, 85], the NxN candidates [band CTUs, 64] or None).  stats: a dict that takes per node `pos` (the winner's position, -1: invalid),
    `second_won`, `planar_won` [nb, 85], `outcome` [nb, 64] (intra_rd_nxn_ref.choose's) and `pu_mode` [nb, 256]"""
    rule = rule or DEFAULT
    P = pic if isinstance(pic, ir.Picture) else ir.Picture(pic, bd)
    cw, ch = (P.W + 63) // 64, (P.H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    modes = np.asarray(modes, np.uint8).reshape(nb, 85, -1)
    at = _per_mode(P, bd, qp, nb, rows)
    out = np.zeros((nb, 85), PDT)
    out[:] = ir.MARKER
    pos = np.full((nb, 85), -1, np.int64)
    second_won = np.zeros((nb, 85), bool)
    planar_won = np.zeros((nb, 85), bool)
    inside = at(0)[0]["part"] != 255   # a node is INSIDE iff it has a record at any mode
    for i in range(nb):
        for k in range(85):
            if not inside[i, k]:
                continue
            count = rule["count"][LEVEL[k]]
            cands = candidates_of(modes[i, k], count, rule["append_planar"])
            if not cands:
                continue
            b, s = best_second([int(at(m)[2][i, k]) for _, m in cands])
            win = b
            if s is not None and int(at(cands[s][1])[1][i, k]) < int(at(cands[b][1])[1][i, k]):   # on the unshifted 64-bit J
                win = s
            p, m = cands[win]
            rec = at(m)[0][i, k].copy()
            rec["pad"] = (m, p)
            out[i, k] = rec
            pos[i, k], second_won[i, k], planar_won[i, k] = p, win == s, p == count
    x = None
    outcome = np.full((nb, nx.NODES8), nx.INVALID, np.int64)
    pu = None
    if modes4 is not None:
        pu = pu_choice(P, bd, qp, np.asarray(modes4, np.uint8).reshape(nb, 256, -1), rule, rows, nb, cw)
        x = nxn_records(P, pu, rows, nb, cw, qp)
        out[:, nx.NODE0:] = nx.choose(out[:, nx.NODE0:], x, outcome)
    if stats is not None:
        stats.update(pos=pos, second_won=second_won, planar_won=planar_won, outcome=outcome, pu_mode=None if pu is None else pu["mode"])
    return out, x


def expected(pic, bd, qp, modes, modes4, rule=None, fold=None, rd_merge=None, skip_mask=0, rows=None, stats=None):
    """one picture -> ([band CTUs, 85] MOTION_RD_PU_DTYPE, [band CTUs, 64] INTRA_RD_NXN_DTYPE or None); fold / rd_merge compact over the same rows, or None"""
    p, x = plain(pic, bd, qp, modes, modes4, rule, rows, stats)
    return ir.gate_fold(p, None if fold is None else fold.reshape(p.shape), None if rd_merge is None else rd_merge.reshape(p.shape), skip_mask), x


same = nx.same


def first_of(modes):
    """records whose modes are the lists' first bytes (identity (i)): [n, K, stride] -> [n, K] NODE_DTYPE with satd 0"""
    a = np.zeros(modes.shape[:2], NDT)
    a["mode"] = modes[:, :, 0]
    return a


# ---- the draw: intra_rd_ref's 35 pictures with node lists and 4x4 lists at stride 8 -----------------------------------------------------------------------------

STRIDE = 8


def random_lists(rng, n, per_ctu):
    """random bytes 0..34 (four in ten: one of 0, 1, 10, 26), one byte in twelve above 34, one entry in sixteen wholly invalid, one in eight with its first byte
    repeated further back"""
    shape = (n, per_ctu, STRIDE)
    special = rng.choice([0, 1, 10, 26], size=shape)
    a = np.where(rng.random(shape) < 0.4, special, rng.integers(0, 35, size=shape))
    a = np.where(rng.random(shape) < 1 / 12, rng.integers(35, 256, size=shape), a)
    a = np.where((rng.random(shape[:2]) < 1 / 16)[..., None], rng.integers(35, 256, size=shape), a)
    dup = rng.random(shape[:2]) < 1 / 8
    at = rng.integers(1, STRIDE, size=shape[:2])
    ii, kk = np.nonzero(dup)
    a[ii, kk, at[ii, kk]] = a[ii, kk, 0]
    return a.astype(np.uint8)


def real_lists(pic, bd, qp):
    """the oracle's own lists of a picture at 8 candidates -> ([numCtus, 85, 8], [numCtus, 256, 8]) uint8; 4x4 PUs outside carry 255"""
    import ctypes as C

    import first_pass_4x4_ref as fp4
    from oracle import oracle_py as op
    lib, _ = ir.oracle()
    H, W = pic.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    flat = np.ascontiguousarray(np.asarray(pic).astype(np.int16)).reshape(-1)
    sl = fp4.sqrt_lambda(lib, qp, bd)
    nodes = np.zeros((cw * ch, 85, STRIDE), np.uint8)
    lib.fho_first_pass_candidates_ctu.restype = None
    for c in range(cw * ch):
        lib.fho_first_pass_candidates_ctu(op.ptr(flat, 0), C.c_int(W), C.c_int(W), C.c_int(H), C.c_int(c % cw), C.c_int(c // cw), C.c_int(bd), C.c_double(sl),
                                          C.c_int(STRIDE), C.c_void_p(nodes[c].ctypes.data))
    return nodes, fp4.expected(lib, flat, 0, W, W, H, bd, qp)["modes"]


@functools.lru_cache(maxsize=None)
def draw(index):
    """entry `index` of intra_rd_ref's DRAW -> dict: bd, qp, pic, modes, modes4, plain, nxn, stats, fold, merge (intra_rd_ref's records)"""
    d = ir.draw(index)
    _, _, seed, real = ir.DRAW[index]
    rng = np.random.default_rng(41000 + seed)
    modes, modes4 = real_lists(d["pic"], d["bd"], d["qp"]) if real else (random_lists(rng, ir.DRAW_N, 85), random_lists(rng, ir.DRAW_N, 256))
    stats = {}
    p, x = plain(d["pic"], d["bd"], d["qp"], modes, modes4, DEFAULT, stats=stats)
    return dict(bd=d["bd"], qp=d["qp"], pic=d["pic"], modes=modes, modes4=modes4, plain=p, nxn=x, stats=stats, fold=d["fold"], merge=d["merge"])
