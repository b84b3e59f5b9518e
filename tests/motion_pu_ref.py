"""numpy restatement of the integer motion search for an arbitrary rectangle (x0, y0, w, h) whose sides are multiples of 8: what
include/fasthevc.h specifies for fhevc_motion_search (squares) and fhevc_motion_search_pu (the rectangular PUs).  Full search over
[-R, R]^2 in a border-replicated reference, raster order with strict "<", SAD or Hadamard SATD summed over the rectangle's 8x8 tiles and
shifted ONCE by bit_depth - 8, plus oracle.fho_mv_cost (getCostOfVectorWithPredictor, zero predictor).

Two forms: the FAST one takes the tile distortions of a whole region per vector and sums them per rectangle (what the kernel does); the DIRECT
one evaluates every vector of one rectangle on the whole w x h block (oracle.fho_satd, pinned to the reference's xGetHADs; a plain sum of
absolute differences for SAD).  tests/test_motion_pu_ref.py pins both."""
import ctypes as C
import math

import numpy as np

MARKER = 0xFFFFFFFF
DT = np.dtype([("satd_zero", np.uint32), ("satd_best", np.uint32), ("cost_best", np.uint32), ("mvx", np.int16), ("mvy", np.int16)])
PUS_PER_CTU = 124
H8 = np.array([[1]], np.int64)
for _ in range(3):
    H8 = np.block([[H8, H8], [H8, -H8]])


def sqrt_lambda(oracle, qp, bd):
    return math.sqrt(oracle.fho_lambda_intra(qp, bd))


def mv_costs(oracle, R, sl):
    """[(2R+1)^2] vector costs in raster order (dy outer, dx inner)"""
    side = 2 * R + 1
    return np.array([oracle.fho_mv_cost(m % side - R, m // side - R, C.c_double(sl)) for m in range(side * side)], np.int64)


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------------

def node_rect(node):
    """(x0, y0, n) of CU node 0..84 inside its CTU"""
    lvl = 0 if node == 0 else 1 if node < 5 else 2 if node < 21 else 3
    ni = node - (0, 1, 5, 21)[lvl]
    n, cnt = 64 >> lvl, 1 << lvl
    return (ni % cnt) * n, (ni // cnt) * n, n


def pu_rect(node, shape, part):
    """(x0, y0, w, h) inside the CTU of part 0 / 1 of HM's PartSize `shape` (0 2NxN, 1 Nx2N, 2 2NxnU, 3 2NxnD, 4 nLx2N, 5 nRx2N) of CU node
    `node`: TComDataCU::getPartIndexAndSize"""
    x0, y0, s = node_rect(node)
    cut = (s // 2, s // 2, s // 4, 3 * s // 4, s // 4, 3 * s // 4)[shape]
    if shape in (0, 2, 3):
        return (x0, y0, s, cut) if part == 0 else (x0, y0 + cut, s, s - cut)
    return (x0, y0, cut, s) if part == 0 else (x0 + cut, y0, s - cut, s)


def pu_index(node, shape, part):
    """the layout include/fasthevc.h states for FHEVC_PUS_PER_CTU, written independently of capi.motion_pu_index"""
    if part not in (0, 1) or shape < 0 or node < 0:
        return -1
    if node <= 4 and shape <= 5:
        return node * 12 + shape * 2 + part
    if 5 <= node <= 20 and shape <= 1:
        return 60 + (node - 5) * 4 + shape * 2 + part
    return -1


def covered():
    """[(node, shape, part)] in output order"""
    out = [(k, s, p) for k in range(5) for s in range(6) for p in range(2)]
    return out + [(k, s, p) for k in range(5, 21) for s in range(2) for p in range(2)]


# ---- distortions ----------------------------------------------------------------------------------------------------------------------------------

def padded(ref, R):
    """the reference with R replicated samples on every side (TComPicYuv::extendPicBorder)"""
    return np.pad(np.asarray(ref, np.int64), R, mode="edge")


def tile_dists(cur, ref, R, sad, x0=0, y0=0, w=None, h=None):
    """[(2R+1)^2, h/8, w/8]: the distortion of every 8x8 tile of region (x0, y0, w, h) of cur at every vector, unshifted: SAD, or
    xCalcHADs8x8's (sum |H d H| + 2) >> 2"""
    cur = np.asarray(cur, np.int64)
    H, W = cur.shape
    w = (W - x0) // 8 * 8 if w is None else w
    h = (H - y0) // 8 * 8 if h is None else h
    rp = padded(ref, R)
    c = cur[y0:y0 + h, x0:x0 + w]
    side = 2 * R + 1
    out = np.zeros((side * side, h // 8, w // 8), np.int64)
    for m in range(side * side):
        dy, dx = m // side - R, m % side - R
        d = c - rp[R + y0 + dy:R + y0 + dy + h, R + x0 + dx:R + x0 + dx + w]
        t = d.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
        if sad:
            out[m] = np.abs(t).sum(axis=(2, 3))
        else:
            out[m] = (np.abs(H8 @ t @ H8).sum(axis=(2, 3)) + 2) >> 2
    return out


def pick(dist, costs, R):
    """dist [(2R+1)^2]: the rectangle's shifted distortion per vector -> one DT record: first raster vector of least cost"""
    side = 2 * R + 1
    cost = dist + costs
    m = int(np.argmin(cost))      # the first minimum in raster order: strict "<"
    r = np.zeros((), DT)
    r["satd_zero"], r["satd_best"], r["cost_best"] = dist[(side * side - 1) // 2], dist[m], cost[m]
    r["mvx"], r["mvy"] = m % side - R, m // side - R
    return r


def search_tiles(td, costs, R, bd, x0, y0, w, h):
    """the fast form: td = tile_dists(...) of a region, (x0, y0, w, h) relative to it, multiples of 8"""
    s = td[:, y0 // 8:(y0 + h) // 8, x0 // 8:(x0 + w) // 8].sum(axis=(1, 2)) >> (bd - 8)
    return pick(s, costs, R)


def search_direct(oracle, cur, ref, costs, R, bd, sad, x0, y0, w, h):
    """the direct form: every vector on the whole w x h block"""
    c = np.ascontiguousarray(np.asarray(cur)[y0:y0 + h, x0:x0 + w], np.int16)
    rp = np.ascontiguousarray(padded(ref, R), np.int16)
    side = 2 * R + 1
    dist = np.zeros(side * side, np.int64)
    for m in range(side * side):
        dy, dx = m // side - R, m % side - R
        if sad:
            dist[m] = int(np.abs(c.astype(np.int64) - rp[R + y0 + dy:R + y0 + dy + h, R + x0 + dx:R + x0 + dx + w]).sum()) >> (bd - 8)
        else:
            off = ((R + y0 + dy) * rp.shape[1] + R + x0 + dx) * 2
            dist[m] = oracle.fho_satd(C.c_void_p(c.ctypes.data), w, C.c_void_p(rp.ctypes.data + off), rp.shape[1], w, h, bd)
    return pick(dist, costs, R)


# ---- whole CTUs -----------------------------------------------------------------------------------------------------------------------------------

def marker():
    r = np.zeros((), DT)
    r["satd_zero"] = r["satd_best"] = r["cost_best"] = MARKER
    return r


def expected(oracle, cur, ref, bd, qp, R, sad, ctus=None):
    """cur, ref: [H, W] samples -> (nodes [numCtus, 85], pus [numCtus, 124]) as the library lays them out; only the CTUs of `ctus` are filled
    (default: all).  A PU is valid iff its CU node lies wholly inside the picture."""
    cur, ref = np.asarray(cur, np.int64), np.asarray(ref, np.int64)
    H, W = cur.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    costs = mv_costs(oracle, R, sqrt_lambda(oracle, qp, bd))
    nodes, pus = np.zeros((cw * ch, 85), DT), np.zeros((cw * ch, PUS_PER_CTU), DT)
    cov = covered()
    for c in (range(cw * ch) if ctus is None else ctus):
        cx, cy = c % cw, c // cw
        w, h = min(64, (W - cx * 64) // 8 * 8), min(64, (H - cy * 64) // 8 * 8)
        td = tile_dists(cur, ref, R, sad, cx * 64, cy * 64, w, h)
        for k in range(85):
            x0, y0, n = node_rect(k)
            nodes[c, k] = search_tiles(td, costs, R, bd, x0, y0, n, n) if x0 + n <= w and y0 + n <= h else marker()
        for i, (k, s, p) in enumerate(cov):
            nx, ny, n = node_rect(k)
            pus[c, i] = search_tiles(td, costs, R, bd, *pu_rect(k, s, p)) if nx + n <= w and ny + n <= h else marker()
    return nodes, pus
