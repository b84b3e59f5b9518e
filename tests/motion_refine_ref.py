"""Expected values of the quarter-sample motion refinement (fhevc_motion_refine*): a numpy restatement of TEncSearch::xPatternSearchFracDIF +
xPatternRefinement as include/fasthevc.h states them -- the sixteen fractional planes of a border-replicated reference picture through HEVC's
8-tap luma filters, the half-sample and the quarter-sample candidate loops in the order of their tables, strict "<", Hadamard distortion from the
CPU oracle's fho_satd and its lambda, the vector cost in quarter units.  Not a test module: tests/test_motion_refine_ref.py pins it without a
GPU, tests/test_gpu_motion_refine.py compares the library with it."""
import ctypes as C
import math

import numpy as np

from fasthevc_amd import capi

MARKER = 0xFFFFFFFF
C1 = (-1, 4, -10, 58, 17, -5, 1, 0)
C2 = (-1, 4, -11, 40, 40, -11, 4, -1)
TAPS = {1: C1, 2: C2, 3: C1[::-1]}       # over samples x-3 .. x+4
# candidate offsets (x, y), centre first; the quarter table's order differs from the half table's
REFINE_H = ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (1, -1), (-1, 1), (1, 1))
REFINE_Q = ((0, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (1, 1))
LEVEL_FIRST = (0, 1, 5, 21)


def sqrt_lambda(oracle, qp, bd):
    return math.sqrt(oracle.fho_lambda_intra(qp, bd))


def eg_bits(v):
    """bits of the signed exp-Golomb code of v"""
    u = ((-v) << 1) + 1 if v <= 0 else v << 1
    return 1 + 2 * (u.bit_length() - 1)


def qpel_cost(qx, qy, sl):
    """getCostOfVectorWithPredictor of a vector in QUARTER samples, zero predictor: fho_mv_cost's arithmetic on the bits of both components"""
    return int((65536.0 * sl * (eg_bits(qx) + eg_bits(qy))) / 65536.0)


def _taps_h(a, c):
    """out[y, x] = sum_k c[k] * a[y, x - 3 + k]; the 3 / 4 columns at the sides that lack taps stay 0 and are never read"""
    out = np.zeros_like(a)
    n = a.shape[1] - 7
    for k in range(8):
        if c[k]:
            out[:, 3:3 + n] += c[k] * a[:, k:k + n]
    return out


def _taps_v(a, c):
    return _taps_h(a.T, c).T


def interpolate(p, fx, fy, bd):
    """the plane of fraction (fx, fy) quarter samples of p (int64 [H, W]): sample [y, x] lies at (x + fx / 4, y + fy / 4)"""
    top = (1 << bd) - 1
    if fx == 0 and fy == 0:
        return p.copy()
    if fy == 0:
        return np.clip((_taps_h(p, TAPS[fx]) + 32) >> 6, 0, top)
    if fx == 0:
        return np.clip((_taps_v(p, TAPS[fy]) + 32) >> 6, 0, top)
    t = (_taps_h(p, TAPS[fx]) >> (bd - 8)) - 8192
    return np.clip((_taps_v(t, TAPS[fy]) + (1 << (19 - bd)) + (8192 << 6)) >> (20 - bd), 0, top)


def vertical_through_intermediate(p, fy, bd):
    """a vertical-only plane the way the reference reaches it: a 14-bit copy (s << (14 - bd)) - 8192, then the second stage of the two-stage form"""
    top = (1 << bd) - 1
    t = (p << (14 - bd)) - 8192
    return np.clip((_taps_v(t, TAPS[fy]) + (1 << (19 - bd)) + (8192 << 6)) >> (20 - bd), 0, top)


class Planes:
    """the sixteen fractional planes [fy][fx] of a reference picture [H, W] replicated `pad` samples beyond every border (extendPicBorder)"""

    def __init__(self, ref_pic, bd, pad):
        self.pad, self.bd = pad, bd
        p = np.pad(np.asarray(ref_pic).astype(np.int64), pad, mode="edge")
        self.width = p.shape[1]
        self.planes = [[np.ascontiguousarray(interpolate(p, fx, fy, bd).astype(np.int16)) for fx in range(4)] for fy in range(4)]

    def block_ptr(self, qx, qy, x0, y0):
        """pointer to the prediction of the block at picture position (x0, y0) displaced by (qx, qy) quarter samples; the row pitch is self.width"""
        a = self.planes[qy & 3][qx & 3]
        return C.c_void_p(a.ctypes.data + 2 * ((self.pad + y0 + (qy >> 2)) * self.width + self.pad + x0 + (qx >> 2)))

    def block(self, qx, qy, x0, y0, n):
        a = self.planes[qy & 3][qx & 3]
        y, x = self.pad + y0 + (qy >> 2), self.pad + x0 + (qx >> 2)
        return a[y:y + n, x:x + n]


def refine_node(oracle, planes, cur_flat, origin, stride, x0, y0, n, mx, my, sl):
    """one node of size n at (x0, y0) with the integer vector (mx, my) -> dict(satd_int, satd_best, cost_best, mvx, mvy, half, quarter):
    half / quarter are the nine (qx, qy, satd, cost) of each stage in table order"""
    cur = C.c_void_p(cur_flat.ctypes.data + 2 * (origin + y0 * stride + x0))

    def stage(base_x, base_y, table, step):
        rows, best = [], None
        for dx, dy in table:
            qx, qy = base_x + step * dx, base_y + step * dy
            satd = int(oracle.fho_satd(cur, stride, planes.block_ptr(qx, qy, x0, y0), planes.width, n, n, planes.bd))
            cost = satd + qpel_cost(qx, qy, sl)
            rows.append((qx, qy, satd, cost))
            if best is None or cost < best[3]:     # strict "<": the first of equal costs in table order wins
                best = rows[-1]
        return rows, best

    half, bh = stage(4 * mx, 4 * my, REFINE_H, 2)
    quarter, bq = stage(bh[0], bh[1], REFINE_Q, 1)
    return dict(satd_int=half[0][2], satd_best=bq[2], cost_best=bq[3], mvx=bq[0], mvy=bq[1], half=half, quarter=quarter)


def node_geometry(k):
    """node index 0..84 -> (level, bx, by)"""
    lvl = 3 if k >= 21 else 2 if k >= 5 else 1 if k >= 1 else 0
    i = k - LEVEL_FIRST[lvl]
    return lvl, i % (1 << lvl), i >> lvl


def expected(oracle, cur_flat, origin, stride, ref_pic, W, H, bd, qp, nodes, max_range, ctus=None, planes=None):
    """cur_flat / origin / stride: the current picture as an int16 plane (frames.to_pel_plane, frames.guarded_plane with poison=None);
    ref_pic: the reference picture's samples [H, W]; nodes: [numCtus, 85] with fields mvx / mvy (integer vectors).
    -> [numCtus, 85] MOTION_QPEL_DTYPE; rows of CTUs not in `ctus` (raster indices, default all) stay zero"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    planes = planes or Planes(ref_pic, bd, max_range + 8)
    assert planes.pad >= max_range + 5 and planes.bd == bd
    sl = sqrt_lambda(oracle, qp, bd)
    out = np.zeros((cw * ch, 85), capi.MOTION_QPEL_DTYPE)
    for c in (range(cw * ch) if ctus is None else ctus):
        cx, cy = c % cw, c // cw
        for k in range(85):
            lvl, bx, by = node_geometry(k)
            n = 64 >> lvl
            x0, y0 = 64 * cx + bx * n, 64 * cy + by * n
            mx, my = int(nodes["mvx"][c, k]), int(nodes["mvy"][c, k])
            if x0 + n > W or y0 + n > H or abs(mx) > max_range or abs(my) > max_range:
                out[c, k] = (MARKER, MARKER, MARKER, 0, 0)
                continue
            r = refine_node(oracle, planes, cur_flat, origin, stride, x0, y0, n, mx, my, sl)
            out[c, k] = (r["satd_int"], r["satd_best"], r["cost_best"], r["mvx"], r["mvy"])
    return out
