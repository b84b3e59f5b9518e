"""Expected values of the merge stage (fhevc_motion_merge*) and of the tree decision that takes its costs (fhevc_p_tree_select_merge*), restated in
Python from the definitions in include/fasthevc.h -- not from the C code: the distortion of a node at one quarter-sample vector (satd_at: the
planes of motion_refine_ref.Planes and the CPU oracle's fho_satd), the candidate list as a function of bare records (build_list), the choice among
its entries, and expected() over a picture and a band.  tests/test_motion_merge_ref.py pins this module without a GPU, tests/test_motion_merge_abi.py
compares the host functions with it, tests/test_gpu_motion_merge.py the kernels.  A plain module, not a conftest and not a test."""
import ctypes as C

import numpy as np

import motion_refine_ref as mr
import p_tree_ref as pt
from fasthevc_amd import capi

MARK = 0xFFFFFFFF
MDT = capi.MOTION_MERGE_DTYPE
L, A, AR, BL, AL, ZERO = 0, 1, 2, 3, 4, 5
OFFSETS = ((-1, 0), (0, -1), (1, -1), (-1, 1), (-1, -1))      # L, A, AR, BL, AL on the level's grid
MERGED = 64                                                   # bit 6 of a tree record's flags
INVALID = (MARK, MARK, 0, 0, 255, 0, 255, 0)                  # the record of a node that is not INSIDE


def z_index(x, y):
    """the bit interleave, x in the even bits"""
    z = 0
    for b in range(3):
        z |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
    return z


def node_index(lvl, bx, by):
    return mr.LEVEL_FIRST[lvl] + by * (1 << lvl) + bx


def inside(W, H, lvl, gx, gy):
    s = 64 >> lvl
    return gx >= 0 and gy >= 0 and (gx + 1) * s <= W and (gy + 1) * s <= H


def key(cw, lvl, gx, gy):
    """coding-order key of the node at grid position (gx, gy) of level lvl: (CTU raster index, z-index inside the CTU)"""
    n = 1 << lvl
    return ((gy >> lvl) * cw + (gx >> lvl), z_index(gx & (n - 1), gy & (n - 1)))


def neighbours(W, H, rows, lvl, gx, gy):
    """the five candidate positions of the node at (gx, gy) -> per position None, or (ctu raster index, node index) of the same-level node there if it lies
    on the grid, is INSIDE, belongs to a CTU row of the band `rows` and precedes the node in coding order"""
    cw = (W + 63) // 64
    n = 1 << lvl
    out = []
    for dx, dy in OFFSETS:
        x, y = gx + dx, gy + dy
        ok = inside(W, H, lvl, x, y) and rows[0] <= (y >> lvl) < rows[1] and key(cw, lvl, x, y) < key(cw, lvl, gx, gy)
        out.append(((y >> lvl) * cw + (x >> lvl), node_index(lvl, x & (n - 1), y & (n - 1))) if ok else None)
    return out


def build_list(cands, max_range):
    """cands: five entries (L, A, AR, BL, AL), each None (no addressable neighbour) or (cost_best, mvx, mvy) of its refined record
    -> the list [(src, (qx, qy)), ...] in HM's order with HM's pruning pairs, closed by the zero vector below five entries"""
    reach = 4 * max_range + 3
    v = [None] * 5                      # the vector of an AVAILABLE candidate
    for j, c in enumerate(cands):
        if c is not None and int(c[0]) != MARK and abs(int(c[1])) <= reach and abs(int(c[2])) <= reach:
            v[j] = (int(c[1]), int(c[2]))
    out = []
    if v[L] is not None:
        out.append((L, v[L]))
    if v[A] is not None and not (v[L] is not None and v[A] == v[L]):
        out.append((A, v[A]))
    if v[AR] is not None and not (v[A] is not None and v[AR] == v[A]):
        out.append((AR, v[AR]))
    if v[BL] is not None and not (v[L] is not None and v[BL] == v[L]):
        out.append((BL, v[BL]))
    if len(out) < 4 and v[AL] is not None and not (v[L] is not None and v[AL] == v[L]) and not (v[A] is not None and v[AL] == v[A]):
        out.append((AL, v[AL]))
    if len(out) < 5:
        out.append((ZERO, (0, 0)))
    return out


def index_bits(i):
    """bits of merge index i with MaxNumMergeCand 5: truncated unary"""
    return 4 if i == 4 else i + 1


def bit_cost(bits, sl):
    """getCost(bits) at the motion lambda: the arithmetic of motion_refine_ref.qpel_cost"""
    return int((65536.0 * sl * bits) / 65536.0)


def choose(entries, satds, sl):
    """entries: build_list's list, satds: the distortion of each -> the record tuple (satd_best, cost_best, mvx, mvy, idx, num, src, pad): strict "<", the
    first entry of equal cost wins"""
    best = None
    for i, ((src, q), sd) in enumerate(zip(entries, satds)):
        cost = sd + bit_cost(index_bits(i), sl)
        if best is None or cost < best[1]:
            best = (sd, cost, q[0], q[1], i, len(entries), src, 0)
    return best


def satd_at(oracle, planes, cur_flat, origin, stride, x0, y0, n, q):
    """xGetHADs of the n x n node at (x0, y0) against the reference displaced by q = (qx, qy) quarter samples"""
    cur = C.c_void_p(cur_flat.ctypes.data + 2 * (origin + y0 * stride + x0))
    return int(oracle.fho_satd(cur, stride, planes.block_ptr(q[0], q[1], x0, y0), planes.width, n, n, planes.bd))


def expected(oracle, cur_flat, origin, stride, ref_pic, W, H, bd, qp, refined, max_range, rows=None, planes=None):
    """refined: [band CTUs, 85] MOTION_QPEL_DTYPE (cost_best, mvx, mvy are read), compact over the CTU rows `rows` (default: the whole picture)
    -> [band CTUs, 85] MOTION_MERGE_DTYPE"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    refined = refined.reshape(nb, 85)
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    assert planes.pad >= max_range + 6 and planes.bd == bd
    sl = mr.sqrt_lambda(oracle, qp, bd)
    out = np.zeros((nb, 85), MDT)
    for i in range(nb):
        c = rows[0] * cw + i
        cx, cy = c % cw, c // cw
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            n = 64 >> lvl
            gx, gy = cx * (1 << lvl) + bx, cy * (1 << lvl) + by
            if not inside(W, H, lvl, gx, gy):
                out[i, k] = INVALID
                continue
            cands = []
            for nb_ in neighbours(W, H, rows, lvl, gx, gy):
                if nb_ is None:
                    cands.append(None)
                else:
                    r = refined[nb_[0] - rows[0] * cw, nb_[1]]
                    cands.append((int(r["cost_best"]), int(r["mvx"]), int(r["mvy"])))
            entries = build_list(cands, max_range)
            satds = [satd_at(oracle, planes, cur_flat, origin, stride, gx * n, gy * n, n, q) for _, q in entries]
            out[i, k] = choose(entries, satds, sl)
    return out


def same(got, exp, what=""):
    """every byte of every record"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    for f in MDT.names:
        bad = got[f] != exp[f]
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())


# ---- the tree decision with merge costs: p_tree_ref extended by the one rule ---------------------------------------------------------------------

def tree_select(shapes, merge, W, H, rows=None, rule=None):
    """shapes / merge: [P, band CTUs, 85] records (or plain integer arrays of cost_best) -> (records, depth_min, depth_max) as p_tree_ref.select: the own
    cost of an INSIDE node is the smaller of the two costs, MARK counting as unavailable -- MARK being the largest value, the plain minimum --, and bit 6
    of an INSIDE node's flags says that the merge cost is strictly smaller"""
    sc = (shapes["cost_best"] if shapes.dtype.names else shapes).astype(np.uint32)
    mc = (merge["cost_best"] if merge.dtype.names else merge).astype(np.uint32)
    rec, dmin, dmax = pt.select(np.minimum(sc, mc), W, H, rows=rows, rule=rule)
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rb = rows[0] if rows is not None else 0
    for i in range(sc.shape[1]):
        vw, vh = pt.valid_size(rb * cw + i, W, H)
        ins = np.array([pt.geometry(k, vw, vh)[0] for k in range(85)])
        rec["flags"][:, i] |= np.where(ins[None, :] & (mc[:, i] < sc[:, i]), MERGED, 0).astype(np.uint8)
    return rec, dmin, dmax


def random_merge(rng, shapes):
    """[P, n, 85] MOTION_MERGE_DTYPE beside p_tree_ref.random_shapes' draw: cost_best a hair around the shape's cost, equal to it, or MARK (half of the time where the shape's is); every other byte
    random -- only cost_best may matter"""
    P, n = shapes.shape[:2]
    a = np.frombuffer(rng.bytes(P * n * 85 * 16), MDT).reshape(P, n, 85).copy()
    sc = shapes["cost_best"].astype(np.int64)
    base = np.where(sc == MARK, rng.integers(50, 5000, size=sc.shape), sc)
    c = np.clip(base + rng.choice([-40, -3, -1, 0, 0, 1, 3, 40], size=sc.shape), 0, MARK - 1)
    c = np.where(rng.random(sc.shape) < np.where(sc == MARK, 0.5, 0.25), MARK, c)      # both unavailable must occur too, roots included
    a["cost_best"] = c.astype(np.uint32)
    return a


def availability_combinations(shapes, merge, W, H, rows=None):
    """per level 0..3 the set of (shape available, merge available) pairs seen on INSIDE nodes"""
    cw = (W + 63) // 64
    rb = rows[0] if rows is not None else 0
    seen = {l: set() for l in range(4)}
    sc, mc = shapes["cost_best"], merge["cost_best"]
    for i in range(sc.shape[1]):
        vw, vh = pt.valid_size(rb * cw + i, W, H)
        for k in range(85):
            if pt.geometry(k, vw, vh)[0]:
                seen[pt.level(k)] |= set(zip((sc[:, i, k] != MARK).tolist(), (mc[:, i, k] != MARK).tolist()))
    return seen
