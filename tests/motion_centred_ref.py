"""Expected values of the coarse motion centres (fhevc_motion_centres*) and of the integer searches around them (fhevc_motion_search_pu_centred*).

Centres: a numpy restatement written directly from the definition in include/fasthevc.h, which has no HM counterpart -- the 4:1 decimated
pictures, the CTU's cells inside the decimated grid, the candidates of [-Rc, Rc]^2 in raster order with strict "<", the whole-sample vector 4 d
priced against a zero predictor at iCostScale 2.  Two forms: `centres` (sliding windows, what the GPU tests compare with) and `centres_literal`
(one Python loop per cell and candidate, what pins the first without a GPU).

Centred search: the SADs of the 4x4 blocks of a CTU at every vector of the sub-window [P - R, P + R] of the +-64 volume that
motion_range_sweep.sad_volume builds (the same arithmetic on that sub-window alone: a CTU costs milliseconds instead of a second), summed per
entry by motion_range_sweep.entry_sums; the winner is the first minimum in raster order of SAD + the cost of d = v - P.

Not a test module: tests/test_motion_centred_ref.py pins it, tests/test_gpu_motion_centred.py holds the kernels to it."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import motion_range_sweep as rs
from fasthevc_amd import capi

DT = capi.MOTION_DTYPE
MARKER = 0xFFFFFFFF
MAX_RC = 14


def sqrt_lambda(qp):
    """sqrt of HM's lambda 0.57 * 2^((qp - 12) / 3) (the oracle's fho_lambda_intra, whatever the bit depth)"""
    return math.sqrt(0.57 * math.pow(2.0, (qp - 12.0) / 3.0))


def bits(v):
    """exp-Golomb bits of the WHOLE-sample component v at iCostScale 2: 2 floor(log2 t) + 1, t = v <= 0 ? (-v << 3) + 1 : v << 3"""
    t = ((-v) << 3) + 1 if v <= 0 else v << 3
    return 2 * (t.bit_length() - 1) + 1


def bit_cost(b, sl):
    """getCost(b): floor(motion lambda * b / 65536) with motion lambda = 65536 sqrt(lambda), in doubles"""
    return int((65536.0 * sl * b) / 65536.0)


def decimate(pic):
    """[H, W] samples -> [H // 4, W // 4]: (sum of the 4x4 samples + 8) >> 4 over the cells wholly inside the picture"""
    p = np.asarray(pic).astype(np.int64)
    gh, gw = p.shape[0] // 4, p.shape[1] // 4
    return (p[:4 * gh, :4 * gw].reshape(gh, 4, gw, 4).sum(axis=(1, 3)) + 8) >> 4


def vector_costs(Rc, sl):
    """[2Rc+1, 2Rc+1] (dy, dx): the cost of the whole-sample vector 4 d"""
    comp = [bits(4 * d) for d in range(-Rc, Rc + 1)]
    return np.array([[bit_cost(by + bx, sl) for bx in comp] for by in comp], np.int64)


def centres(cur, ref, bd, sl, Rc):
    """one record per CTU in raster order"""
    assert 1 <= Rc <= MAX_RC
    H, W = np.asarray(cur).shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    Dc, Dr = decimate(cur), decimate(ref)
    gh, gw = Dc.shape
    out = np.zeros(cw * ch, DT)
    vc = vector_costs(Rc, sl)
    S = 2 * Rc + 1
    Drp = np.pad(Dr, Rc, mode="edge") if gw and gh else None
    for c in range(cw * ch):
        cx, cy = c % cw, c // cw
        vw, vh = min(16, gw - 16 * cx), min(16, gh - 16 * cy)
        o = out[c]
        if vw <= 0 or vh <= 0:
            o["satd_zero"] = o["satd_best"] = o["cost_best"] = MARKER
            continue
        cells = Dc[16 * cy:16 * cy + vh, 16 * cx:16 * cx + vw]
        win = Drp[16 * cy:16 * cy + vh + 2 * Rc, 16 * cx:16 * cx + vw + 2 * Rc]      # padded by Rc: candidate (dy, dx) starts at (dy + Rc, dx + Rc)
        sad = (16 * np.abs(sliding_window_view(win, (vh, vw)) - cells).sum(axis=(2, 3))) >> (bd - 8)
        assert sad.shape == (S, S)
        cost = sad + vc
        m = int(np.argmin(cost.reshape(-1)))      # the first minimum in raster order: strict "<"
        o["satd_zero"], o["satd_best"], o["cost_best"] = sad[Rc, Rc], sad.reshape(-1)[m], cost.reshape(-1)[m]
        o["mvx"], o["mvy"] = 4 * (m % S - Rc), 4 * (m // S - Rc)
    return out


def centres_literal(cur, ref, bd, sl, Rc, ctus=None):
    """the same, one cell and one candidate at a time (slow: small pictures only)"""
    cur, ref = np.asarray(cur).astype(np.int64), np.asarray(ref).astype(np.int64)
    H, W = cur.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    gw, gh = W // 4, H // 4

    def D(p, X, Y):
        X, Y = min(max(X, 0), gw - 1), min(max(Y, 0), gh - 1)
        return (int(p[4 * Y:4 * Y + 4, 4 * X:4 * X + 4].sum()) + 8) >> 4

    out = np.zeros(cw * ch, DT)
    for c in (range(cw * ch) if ctus is None else ctus):
        cx, cy = c % cw, c // cw
        own = [(16 * cx + i, 16 * cy + j) for j in range(16) for i in range(16) if 16 * cx + i < gw and 16 * cy + j < gh]
        o = out[c]
        if not own:
            o["satd_zero"] = o["satd_best"] = o["cost_best"] = MARKER
            continue
        dc = {xy: D(cur, *xy) for xy in own}
        best = None
        for dy in range(-Rc, Rc + 1):
            for dx in range(-Rc, Rc + 1):
                sad = (16 * sum(abs(dc[(X, Y)] - D(ref, X + dx, Y + dy)) for X, Y in own)) >> (bd - 8)
                cost = sad + bit_cost(bits(4 * dx) + bits(4 * dy), sl)
                if dx == 0 and dy == 0:
                    o["satd_zero"] = sad
                if best is None or cost < best[0]:
                    best = (cost, sad, 4 * dx, 4 * dy)
        o["cost_best"], o["satd_best"], o["mvx"], o["mvy"] = best
    return out


# ---- the integer searches around a centre ------------------------------------------------------------------------------------------------------------

CENTRE_MAX = 56
FAMS, PER = rs.FAMS, rs.PER


def centred_volume(cur, ref, x0, y0, w, h, px, py, R):
    """[h/4, w/4, 2R+1, 2R+1]: motion_range_sweep.sad_volume's rows and columns (py - R .. py + R, px - R .. px + R) of the +-64 volume, |p| + R <= 64"""
    assert w % 4 == 0 and h % 4 == 0 and abs(px) + R <= rs.MAXR and abs(py) + R <= rs.MAXR
    S, M = 2 * R + 1, rs.MAXR
    rpad = np.pad(np.asarray(ref).astype(np.int64), M, mode="edge")
    c = np.asarray(cur)[y0:y0 + h, x0:x0 + w].astype(np.int64)
    out = np.empty((h // 4, w // 4, S, S), np.int32)
    for dy in range(S):
        rows = rpad[M + y0 + py - R + dy:M + y0 + py - R + dy + h, M + x0 + px - R:M + x0 + px + R + w]
        d = np.abs(sliding_window_view(rows, w, axis=1) - c[:, None, :])          # [h, S, w]: d[y, dx, x]
        out[:, :, dy, :] = d.reshape(h // 4, 4, S, w // 4, 4).sum(axis=(1, 4)).transpose(0, 2, 1)
    return out


def centred_search(oracle, cur, ref, bd, qp, R, centres, ctus=None):
    """{family: [numCtus, per CTU]} records with absolute vectors; centres: [numCtus] with mvx / mvy; CTUs not in `ctus` stay zero"""
    cur, ref = np.asarray(cur, np.int64), np.asarray(ref, np.int64)
    H, W = cur.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    valid = rs.valid_entries(W, H)
    costs = rs.cost_window(oracle, R, rs.mp.sqrt_lambda(oracle, qp, bd)).reshape(-1)
    S = 2 * R + 1
    out = {f: np.zeros((cw * ch, PER[f]), DT) for f in FAMS}
    for c in (range(cw * ch) if ctus is None else ctus):
        px, py = int(centres["mvx"][c]), int(centres["mvy"][c])
        for f in FAMS:
            r = out[f][c]
            r["satd_zero"], r["satd_best"], r["cost_best"] = MARKER, MARKER, MARKER
        if abs(px) > CENTRE_MAX or abs(py) > CENTRE_MAX:
            continue
        x0, y0 = 64 * (c % cw), 64 * (c // cw)
        w, h = min(64, W - x0) // 4 * 4, min(64, H - y0) // 4 * 4
        if w == 0 or h == 0:
            continue
        I = rs.integral(centred_volume(cur, ref, x0, y0, w, h, px, py, R))
        for f in FAMS:
            ok = np.flatnonzero(valid[f][c])
            if not len(ok):
                continue
            E = rs.entry_sums(I, [rs.ENTRIES[f][i][1:] for i in ok], bd - 8).reshape(len(ok), S * S).astype(np.int64)
            total = E + costs[None, :]
            m = np.argmin(total, axis=1)          # the first minimum in raster order over d: strict "<"
            r = np.zeros(len(ok), DT)
            r["satd_zero"], r["satd_best"], r["cost_best"] = E[:, (S * S - 1) // 2], E[np.arange(len(ok)), m], total[np.arange(len(ok)), m]
            r["mvx"], r["mvy"] = px + m % S - R, py + m // S - R
            out[f][c, ok] = r
    return out


# ---- the quarter-sample refinements around a centre -----------------------------------------------------------------------------------------------------

QDT = capi.MOTION_QPEL_DTYPE


def refine_block_centred(oracle, planes, cur_flat, stride, x0, y0, w, h, mx, my, px, py, sl):
    """motion_refine_ref.refine_node / motion_refine_pu_ref.refine_block (one definition: fho_satd takes the branch xGetHADs takes for w x h) with the vector
    cost re-based on the predictor 4 P -> (satd_int, satd_best, cost_best, mvx, mvy)"""
    import ctypes as C
    cur = C.c_void_p(cur_flat.ctypes.data + 2 * (y0 * stride + x0))

    def stage(base_x, base_y, table, step, first=None):
        best = None
        for dx, dy in table:
            qx, qy = base_x + step * dx, base_y + step * dy
            satd = int(oracle.fho_satd(cur, stride, planes.block_ptr(qx, qy, x0, y0), planes.width, w, h, planes.bd))
            cost = satd + rs.mr.qpel_cost(qx - 4 * px, qy - 4 * py, sl)
            if first is not None and not first:
                first.append(satd)
            if best is None or cost < best[3]:     # strict "<": the first of equal costs in table order wins
                best = (qx, qy, satd, cost)
        return best

    at_int = []
    bh = stage(4 * mx, 4 * my, rs.mr.REFINE_H, 2, at_int)
    bq = stage(bh[0], bh[1], rs.mr.REFINE_Q, 1)
    return at_int[0], bq[2], bq[3], bq[0], bq[1]


def centred_refine(oracle, cur, ref, bd, qp, max_range, centres, ins, ctus=None, planes=None):
    """ins: {family: [numCtus, per CTU]} with absolute mvx / mvy -> the same shapes of MOTION_QPEL_DTYPE; CTUs not in `ctus` stay zero"""
    cur = np.asarray(cur, np.int64)
    H, W = cur.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    valid = rs.valid_entries(W, H)
    sl = rs.mr.sqrt_lambda(oracle, qp, bd)
    planes = planes or rs.mr.Planes(ref, bd, rs.MAXR + 8)
    cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
    out = {}
    for f, a in ins.items():
        o = np.zeros(a.shape, QDT)
        for c in (range(cw * ch) if ctus is None else ctus):
            px, py = int(centres["mvx"][c]), int(centres["mvy"][c])
            ok_c = abs(px) <= CENTRE_MAX and abs(py) <= CENTRE_MAX
            for i, (_, x0, y0, w, h) in enumerate(rs.ENTRIES[f]):
                mx, my = int(a["mvx"][c, i]), int(a["mvy"][c, i])
                if not (valid[f][c, i] and ok_c and abs(mx - px) <= max_range and abs(my - py) <= max_range):
                    o[c, i] = (MARKER, MARKER, MARKER, 0, 0)
                else:
                    o[c, i] = refine_block_centred(oracle, planes, cur_flat, W, x0 + 64 * (c % cw), y0 + 64 * (c // cw), w, h, mx, my, px, py, sl)
        out[f] = o
    return out


def make_centres(vectors):
    """[(x, y)] per CTU -> [numCtus] records of which only mvx / mvy mean anything (the rest is filled with a pattern the searches must not read)"""
    a = np.zeros(len(vectors), DT)
    a["satd_zero"], a["satd_best"], a["cost_best"] = 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF
    a["mvx"], a["mvy"] = [v[0] for v in vectors], [v[1] for v in vectors]
    return a


# ---- constructed content ----------------------------------------------------------------------------------------------------------------------------

def texture(W, H, bd, seed, margin=64):
    """[H + 2 margin, W + 2 margin] band-limited random texture: random levels on an 8-sample grid, so that the 4:1 decimation keeps its contrast"""
    rng = np.random.default_rng(seed)
    h, w = H + 2 * margin, W + 2 * margin
    return rng.integers(0, 1 << bd, size=(h // 8 + 1, w // 8 + 1)).repeat(8, 0).repeat(8, 1)[:h, :w].astype(np.int64)


def panned_pair(W, H, bd, seed, vx, vy, margin=64):
    """(cur, ref) with cur(x, y) = ref(x + vx, y + vy) wherever that lies inside ref: the vector a search of cur in ref finds is (vx, vy)"""
    big = texture(W, H, bd, seed, margin)
    assert abs(vx) <= margin and abs(vy) <= margin
    return big[margin + vy:margin + vy + H, margin + vx:margin + vx + W], big[margin:margin + H, margin:margin + W]


# ---- the reference's own results (tests/golden/ref_motion_centred.npz, written by tests/quality/gen_motion_centred_golden.py) -------------------------------

GOLDEN = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "ref_motion_centred.npz")
SLICES = {"nodes": slice(0, 85), "pu": slice(85, 209), "small": slice(209, 593)}      # the file's entry order: 85 + 124 + 384 per CTU


class GoldenCase:
    """one case of the file: planes, centres [numCtus] (MOTION_DTYPE), the five recorded CTUs, and per family the reference's records of those CTUs with the
    flags of the entries whose every read stays inside the picture (the only ones the library and the reference agree on by construction)"""

    def __init__(self, z, k):
        self.k = k
        self.bd, self.qp, self.R, p = (int(v) for v in z["cases"][k])
        self.W, self.H = (int(v) for v in z["size"])
        self.cur, self.ref = z[f"cur{p}"].astype(np.int64), z[f"ref{p}"].astype(np.int64)
        self.ctus = [int(c) for c in z["ctus"]]
        self.centres = make_centres([tuple(int(v) for v in c) for c in z[f"centres{k}"]])
        self.counts = dict(zip(FAMS, (int(v) for v in z["counts"][k])))
        self.counts_frac = dict(zip(FAMS, (int(v) for v in z["counts_frac"][k])))
        res, vin, frac = z[f"res{k}"], z[f"in{k}"], z[f"frac{k}"]
        self.inside = {f: z[f"inside{k}"][:, s] for f, s in SLICES.items()}
        self.inside_frac = {f: z[f"inside_frac{k}"][:, s] for f, s in SLICES.items()}
        self.search, self.vin, self.frac = {}, {}, {}
        for f, s in SLICES.items():
            a = np.zeros(res[:, s].shape[:2], DT)
            a["mvx"], a["mvy"], a["satd_best"], a["cost_best"], a["satd_zero"] = (res[:, s, i] for i in range(5))
            self.search[f] = a
            v = np.zeros(a.shape, DT)
            v["mvx"], v["mvy"] = vin[:, s, 0], vin[:, s, 1]
            self.vin[f] = v
            q = np.zeros(a.shape, QDT)
            q["satd_int"], q["satd_best"], q["cost_best"], q["mvx"], q["mvy"] = (frac[:, s, i] for i in range(5))
            self.frac[f] = q

    def full_inputs(self):
        """{family: [numCtus, per CTU]}: the refinement's input vectors, the file's in the recorded CTUs, the centre elsewhere"""
        out = {}
        for f in FAMS:
            a = np.zeros((len(self.centres), PER[f]), DT)
            a["mvx"], a["mvy"] = self.centres["mvx"][:, None], self.centres["mvy"][:, None]
            a[self.ctus] = self.vin[f]
            out[f] = a
        return out

    def __repr__(self):
        return f"golden case {self.k}: {self.bd} bit, QP {self.qp}, R {self.R}"


def golden_cases():
    z = np.load(GOLDEN)
    return [GoldenCase(z, k) for k in range(len(z["cases"]))]


def same_flagged(got, exp, flags, names, what=""):
    """got, exp [5, per CTU] records; every field of the flagged entries -> how many were compared"""
    for n in names:
        bad = (got[n] != exp[n]) & flags
        assert not bad.any(), (what, n, np.argwhere(bad)[:5], got[n][bad][:5], exp[n][bad][:5])
    return int(flags.sum())
