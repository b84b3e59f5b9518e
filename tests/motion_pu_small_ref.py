"""numpy restatement of the integer motion search of the PUs with a 4-sample side: what include/fasthevc.h specifies for
fhevc_motion_search_pu_small.  The AMP shapes of the 16x16 CUs (16x4, 16x12, 4x16, 12x16) and the 2NxN / Nx2N PUs of the 8x8 CUs (8x4, 4x8):
full search over [-R, R]^2 in a border-replicated reference, raster order with strict "<", plus oracle.fho_mv_cost (zero predictor).  The
distortion of such a block is NOT built from 8x8 tiles: TComRdCost::xGetHADs sends a block with a side that is no multiple of 8 wholly through
xCalcHADs4x4, so SATD is the sum over all its 4x4 tiles of (sum |H4 d H4| + 1) >> 1, shifted ONCE by bit_depth - 8; SAD is the plain sum,
shifted once.

Two forms: the QUADRANT one takes the 4x4 distortions of a whole region per vector and sums them per PU (what the kernel does); the DIRECT one
is motion_pu_ref.search_direct: every vector of one PU on the whole w x h block (oracle.fho_satd, pinned to the reference's xGetHADs on the 4x4
branch; a plain sum of absolute differences for SAD).  tests/test_motion_pu_small_ref.py pins both.  Geometry, vector costs and the choice of
the winner are motion_pu_ref's."""
import numpy as np

from motion_pu_ref import DT, MARKER, marker, mv_costs, node_rect, padded, pick, pu_rect, search_direct, sqrt_lambda  # noqa: F401

PUS_SMALL_PER_CTU = 384
H4 = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], np.int64)


def pu_small_index(node, shape, part):
    """the layout include/fasthevc.h states for FHEVC_PUS_SMALL_PER_CTU, written independently of capi.motion_pu_small_index"""
    if part not in (0, 1):
        return -1
    if 5 <= node <= 20 and 2 <= shape <= 5:
        return 8 * (node - 5) + 2 * (shape - 2) + part
    if 21 <= node <= 84 and 0 <= shape <= 1:
        return 128 + 4 * (node - 21) + 2 * shape + part
    return -1


def covered():
    """[(node, shape, part)] in output order"""
    out = [(k, s, p) for k in range(5, 21) for s in range(2, 6) for p in range(2)]
    return out + [(k, s, p) for k in range(21, 85) for s in range(2) for p in range(2)]


def quad_dists(cur, ref, R, sad, x0=0, y0=0, w=None, h=None):
    """[(2R+1)^2, h/4, w/4]: the distortion of every 4x4 tile of region (x0, y0, w, h) of cur at every vector, unshifted: SAD, or
    xCalcHADs4x4's (sum |H d H| + 1) >> 1"""
    cur = np.asarray(cur, np.int64)
    H, W = cur.shape
    w = (W - x0) // 4 * 4 if w is None else w
    h = (H - y0) // 4 * 4 if h is None else h
    rp = padded(ref, R)
    c = cur[y0:y0 + h, x0:x0 + w]
    side = 2 * R + 1
    out = np.zeros((side * side, h // 4, w // 4), np.int64)
    for m in range(side * side):
        dy, dx = m // side - R, m % side - R
        d = c - rp[R + y0 + dy:R + y0 + dy + h, R + x0 + dx:R + x0 + dx + w]
        t = d.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3)
        if sad:
            out[m] = np.abs(t).sum(axis=(2, 3))
        else:
            out[m] = (np.abs(H4 @ t @ H4).sum(axis=(2, 3)) + 1) >> 1
    return out


def quad_sum(qd, bd, x0, y0, w, h):
    """[(2R+1)^2]: the distortion of block (x0, y0, w, h), relative to qd's region and in multiples of 4, per vector: the sum of its 4x4 tiles,
    shifted once"""
    return qd[:, y0 // 4:(y0 + h) // 4, x0 // 4:(x0 + w) // 4].sum(axis=(1, 2)) >> (bd - 8)


def search_quads(qd, costs, R, bd, x0, y0, w, h):
    """the quadrant form: qd = quad_dists(...) of a region"""
    return pick(quad_sum(qd, bd, x0, y0, w, h), costs, R)


def expected(oracle, cur, ref, bd, qp, R, sad, ctus=None):
    """cur, ref: [H, W] samples -> pus [numCtus, 384] as the library lays them out; only the CTUs of `ctus` are filled (default: all).  A PU is
    valid iff its CU node lies wholly inside the picture."""
    cur, ref = np.asarray(cur, np.int64), np.asarray(ref, np.int64)
    H, W = cur.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    costs = mv_costs(oracle, R, sqrt_lambda(oracle, qp, bd))
    pus = np.zeros((cw * ch, PUS_SMALL_PER_CTU), DT)
    cov = covered()
    for c in (range(cw * ch) if ctus is None else ctus):
        cx, cy = c % cw, c // cw
        w, h = min(64, W - cx * 64), min(64, H - cy * 64)
        qd = quad_dists(cur, ref, R, sad, cx * 64, cy * 64, w // 4 * 4, h // 4 * 4)
        for i, (k, s, p) in enumerate(cov):
            nx, ny, n = node_rect(k)
            pus[c, i] = search_quads(qd, costs, R, bd, *pu_rect(k, s, p)) if nx + n <= w and ny + n <= h else marker()
    return pus
