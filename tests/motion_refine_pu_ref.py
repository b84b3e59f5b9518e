"""Expected values of the quarter-sample refinement of the PUs' vectors (fhevc_motion_refine_pu*): motion_refine_ref.refine_node for an arbitrary
w x h block -- the same two candidate loops, the same fractional planes and vector cost, the distortion from the CPU oracle's fho_satd on the
WHOLE block, which takes xGetHADs' own branch: 8x8 Hadamards if both sides are multiples of 8, else 4x4 Hadamards over the whole block, the
block's sum shifted once.  PU geometry and entry order come from motion_pu_ref (the 124) and motion_pu_small_ref (the 384).  Not a test module:
tests/test_motion_refine_pu_ref.py pins it without a GPU, tests/test_gpu_motion_refine_pu.py compares the library with it."""
import ctypes as C

import numpy as np

import motion_pu_ref as mp
import motion_pu_small_ref as ps
from fasthevc_amd import capi
from motion_refine_ref import MARKER, REFINE_H, REFINE_Q, Planes, qpel_cost, sqrt_lambda  # noqa: F401

FAMILIES = {"pu": (mp.covered, mp.PUS_PER_CTU), "small": (ps.covered, ps.PUS_SMALL_PER_CTU)}


def refine_block(oracle, planes, cur_flat, origin, stride, x0, y0, w, h, mx, my, sl):
    """one w x h block at (x0, y0) with the integer vector (mx, my) -> dict(satd_int, satd_best, cost_best, mvx, mvy, half, quarter): half /
    quarter are the nine (qx, qy, satd, cost) of each stage in table order"""
    cur = C.c_void_p(cur_flat.ctypes.data + 2 * (origin + y0 * stride + x0))

    def stage(base_x, base_y, table, step):
        rows, best = [], None
        for dx, dy in table:
            qx, qy = base_x + step * dx, base_y + step * dy
            satd = int(oracle.fho_satd(cur, stride, planes.block_ptr(qx, qy, x0, y0), planes.width, w, h, planes.bd))
            cost = satd + qpel_cost(qx, qy, sl)
            rows.append((qx, qy, satd, cost))
            if best is None or cost < best[3]:     # strict "<": the first of equal costs in table order wins
                best = rows[-1]
        return rows, best

    half, bh = stage(4 * mx, 4 * my, REFINE_H, 2)
    quarter, bq = stage(bh[0], bh[1], REFINE_Q, 1)
    return dict(satd_int=half[0][2], satd_best=bq[2], cost_best=bq[3], mvx=bq[0], mvy=bq[1], half=half, quarter=quarter)


def expected(oracle, cur, ref, bd, qp, pus, max_range, family, ctus=None, planes=None):
    """cur, ref: [H, W] samples; pus: [numCtus, 124] (family "pu") or [numCtus, 384] (family "small") with fields mvx / mvy (integer vectors)
    -> the same shape of MOTION_QPEL_DTYPE; rows of CTUs not in `ctus` (raster indices, default all) stay zero.  A PU is valid iff its CU node
    lies wholly inside the picture and |mvx|, |mvy| <= max_range.  planes: the fractional planes of the whole reference (default: per CTU, of the
    CTU's surroundings only -- no candidate reaches further than max_range + 1 + 4 taps beyond the CTU, so a large picture costs no more per CTU)"""
    covered, per_ctu = FAMILIES[family]
    cur, ref = np.asarray(cur), np.asarray(ref)
    H, W = cur.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    assert pus.shape == (cw * ch, per_ctu)
    m = max_range + 8
    assert planes is None or (planes.pad >= max_range + 5 and planes.bd == bd)
    sl = sqrt_lambda(oracle, qp, bd)
    out = np.zeros((cw * ch, per_ctu), capi.MOTION_QPEL_DTYPE)
    cov = covered()
    for c in (range(cw * ch) if ctus is None else ctus):
        cx, cy = c % cw, c // cw
        # the crop's edges are the picture's (replicated by Planes, as extendPicBorder does) or lie beyond every sample a candidate reads
        xl, yl = (0, 0) if planes else (max(0, 64 * cx - m), max(0, 64 * cy - m))
        xh, yh = (W, H) if planes else (min(W, 64 * cx + 64 + m), min(H, 64 * cy + 64 + m))
        pl = planes or Planes(ref[yl:yh, xl:xh], bd, m)
        flat = np.ascontiguousarray(cur[yl:yh, xl:xh].astype(np.int16)).reshape(-1)
        for i, (k, s, p) in enumerate(cov):
            nx, ny, n = mp.node_rect(k)
            mx, my = int(pus["mvx"][c, i]), int(pus["mvy"][c, i])
            if 64 * cx + nx + n > W or 64 * cy + ny + n > H or abs(mx) > max_range or abs(my) > max_range:
                out[c, i] = (MARKER, MARKER, MARKER, 0, 0)
                continue
            x0, y0, w, h = mp.pu_rect(k, s, p)
            r = refine_block(oracle, pl, flat, 0, xh - xl, 64 * cx + x0 - xl, 64 * cy + y0 - yl, w, h, mx, my, sl)
            out[c, i] = (r["satd_int"], r["satd_best"], r["cost_best"], r["mvx"], r["mvy"])
    return out


# ---- a picture built by the filter itself: two half-sample motions inside one CU -------------------------------------------------------------------

# kind -> (family, shape, the CU nodes it is about, first(xx, yy): the samples of part 0, coordinates inside the CTU)
TWO_MOTION_KINDS = {
    "2NxnU@16": ("small", 2, range(5, 21), lambda xx, yy: yy % 16 < 4),
    "nLx2N@16": ("small", 4, range(5, 21), lambda xx, yy: xx % 16 < 4),
    "2NxN@8": ("small", 0, range(21, 85), lambda xx, yy: yy % 8 < 4),
    "Nx2N@8": ("small", 1, range(21, 85), lambda xx, yy: xx % 8 < 4),
    "2NxN@32": ("pu", 0, range(1, 5), lambda xx, yy: yy % 32 < 16),
}


def two_motion_picture(planes, kinds, qa, qb):
    """[64, 64 * len(kinds)]: CTU i holds, in part 0 of every CU of TWO_MOTION_KINDS[kinds[i]], the reference displaced by qa (quarter samples),
    elsewhere by qb -- samples taken from the fractional planes themselves, so the prediction at the true vector equals them exactly"""
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


def two_motion_inputs(kinds, family, a, b):
    """[len(kinds), 124 or 384] integer vectors: a in every part 0, b in every part 1"""
    covered, per_ctu = FAMILIES[family]
    pus = np.zeros((len(kinds), per_ctu), capi.MOTION_DTYPE)
    part = np.array([p for _, _, p in covered()])
    pus["mvx"], pus["mvy"] = np.where(part == 0, a[0], b[0]), np.where(part == 0, a[1], b[1])
    return pus
