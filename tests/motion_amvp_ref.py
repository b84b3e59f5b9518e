"""Expected values of the re-pricing against neighbour predictors (fhevc_motion_amvp*), restated in Python from the definition in include/fasthevc.h -- not
from the C code.  Geometry, candidate samples and the same-level nodes that hold them are motion_merge_pu_ref's (samples, pu_geometry, candidates) and
motion_merge_ref's (neighbours, keys); what this module adds is the own-CU rule (part 1 of a PU sees part 0 of the same partition size), the list of two, eg,
the choice and the saturation.  tests/test_motion_amvp_ref.py pins this module without a GPU, tests/test_motion_amvp_abi.py compares the host twin with it,
tests/test_gpu_motion_amvp.py the kernel.  A plain module, not a conftest and not a test."""
import collections
import math

import numpy as np

import motion_merge_pu_ref as mpr
import motion_merge_ref as mg
import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_refine_ref as mr
from fasthevc_amd import capi

MARK, SAT = 0xFFFFFFFF, 0xFFFFFFFE
QDT, VDT = capi.MOTION_QPEL_DTYPE, capi.MOTION_MVP_DTYPE
L, A, AR, BL, AL, ZERO = 0, 1, 2, 3, 4, 5
PER = {"nodes": 85, "pu": 124, "small": 384}
NO_PRICE = (0, 0, 255, 0, 255, 0)            # the predictor record of a marker entry and of an entry that is not INSIDE
MARKER = (MARK, MARK, MARK, 0, 0)            # the refinement's marker record
BIT_COSTS = 67


def covered(family):
    """[(node, shape or None, part)] in the family's output order"""
    return [(k, None, 0) for k in range(85)] if family == "nodes" else (mp.covered() if family == "pu" else ps.covered())


def sqrt_lambda(qp):
    """sqrt of 0.57 * 2^((qp - 12) / 3): the motion lambda does not depend on the bit depth"""
    return math.sqrt(0.57 * math.pow(2.0, (qp - 12.0) / 3.0))


def eg(v):
    """xGetExpGolombNumberOfBits at cost scale 0"""
    t = ((-v) << 1) + 1 if v <= 0 else v << 1
    return 2 * (t.bit_length() - 1) + 1


def cost_table(qp):
    """c[b] = getCost(b), b = 0..66"""
    return [mg.bit_cost(b, sqrt_lambda(qp)) for b in range(BIT_COSTS)]


def build_list(cands):
    """cands: five entries (L, A, AR, BL, AL), each None or the vector (x, y) of an AVAILABLE candidate -> (the list of two [(src, vector)], num_spatial)"""
    a = next(((j, cands[j]) for j in (BL, L) if cands[j] is not None), None)
    b = next(((j, cands[j]) for j in (AR, A, AL) if cands[j] is not None), None)
    lst = [x for x in (a, b) if x is not None]
    if len(lst) == 2 and lst[0][1] == lst[1][1]:
        lst.pop()
    n = len(lst)
    while len(lst) < 2:
        lst.append((ZERO, (0, 0)))
    return lst, n


def choose(q, lst):
    """q: the entry's vector -> (idx, bits of both entries): the first index of least bits"""
    bits = [eg(q[0] - p[0]) + eg(q[1] - p[1]) for _, p in lst]
    return (1 if bits[1] < bits[0] else 0), bits


def positions(W, H, rows, c, k, s, p):
    """the five positions of entry (node k, shape s or None, part p) of CTU c -> None where the entry's CU node is not INSIDE, otherwise per position None,
    ("own",) -- the sample lies inside the entry's own CU: part 0 of the same partition size -- or ("node", ctu raster index, node index)"""
    cw = (W + 63) // 64
    if s is None:
        lvl, bx, by = mr.node_geometry(k)
        gx, gy = (c % cw) * (1 << lvl) + bx, (c // cw) * (1 << lvl) + by
        if not mg.inside(W, H, lvl, gx, gy):
            return None
        return [None if nb is None else ("node",) + nb for nb in mg.neighbours(W, H, rows, lvl, gx, gy)]
    lvl, (gx, gy), rect = mpr.pu_geometry(W, c, k, s, p)
    if not mg.inside(W, H, lvl, gx, gy):
        return None
    size = 64 >> lvl
    out = []
    for (sx, sy), nb in zip(mpr.samples(*rect), mpr.candidates(W, H, rows, c, k, s, p)):
        if gx * size <= sx < (gx + 1) * size and gy * size <= sy < (gy + 1) * size:
            assert nb is None                     # its key equals the entry's own: the merge rule never takes it
            out.append(("own",))
        else:
            out.append(None if nb is None else ("node",) + nb)
    return out


_PLANS = {}


def plan(W, H, rows, family):
    """per band CTU and entry of the family: positions(); computed once per geometry"""
    key = (W, H, tuple(rows), family)
    if key not in _PLANS:
        cw = (W + 63) // 64
        cov = covered(family)
        _PLANS[key] = [[positions(W, H, rows, rows[0] * cw + i, k, s, p) for k, s, p in cov] for i in range((rows[1] - rows[0]) * cw)]
    return _PLANS[key]


def expected(W, H, nodes, entries, family, qp, rows=None, stats=None):
    """nodes [band CTUs, 85], entries [band CTUs, 85 / 124 / 384] MOTION_QPEL_DTYPE (entries is nodes for family "nodes"), compact over the CTU rows `rows`
    -> (re-priced records, predictor records).  stats: a dict of Counters keyed by level, filled with what happened (see OUTCOMES)"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb, per = (rows[1] - rows[0]) * cw, PER[family]
    nodes, entries = nodes.reshape(nb, 85), entries.reshape(nb, per)
    c = cost_table(qp)
    cov = covered(family)
    part0 = {e: cov.index((k, s, 0)) for e, (k, s, p) in enumerate(cov) if p == 1}
    n_cost, n_x, n_y = nodes["cost_best"].tolist(), nodes["mvx"].tolist(), nodes["mvy"].tolist()
    e_cost, e_x, e_y, e_satd = entries["cost_best"].tolist(), entries["mvx"].tolist(), entries["mvy"].tolist(), entries["satd_best"].tolist()
    out, mvp = entries.copy(), np.zeros((nb, per), VDT)
    for i, per_ctu in enumerate(plan(W, H, rows, family)):
        for e, pos in enumerate(per_ctu):
            if pos is None:
                out[i, e], mvp[i, e] = MARKER, NO_PRICE
                continue
            if e_cost[i][e] == MARK:
                mvp[i, e] = NO_PRICE              # the record is copied as it is
                continue
            cands, own = [], False
            for where in pos:
                if where is None:
                    cands.append(None)
                elif where[0] == "own":
                    e0 = part0[e]
                    own = own or e_cost[i][e0] != MARK
                    cands.append((e_x[i][e0], e_y[i][e0]) if e_cost[i][e0] != MARK else None)
                else:
                    j, kn = where[1] - rows[0] * cw, where[2]
                    cands.append((n_x[j][kn], n_y[j][kn]) if n_cost[j][kn] != MARK else None)
            lst, n = build_list(cands)
            q = (e_x[i][e], e_y[i][e])
            idx, bits = choose(q, lst)
            total = e_satd[i][e] + c[bits[idx]]
            out["cost_best"][i, e] = min(total, SAT)
            mvp[i, e] = (lst[idx][1][0], lst[idx][1][1], idx, n, lst[idx][0], bits[idx])
            if stats is not None:
                lvl = mr.node_geometry(cov[e][0])[0]
                seen = stats.setdefault(lvl, collections.Counter())
                seen["num_spatial_%d" % n] += 1
                seen["src_%d" % lst[idx][0]] += 1
                seen["idx_1"] += idx
                seen["dedupe"] += any(cands[j] is not None for j in (BL, L)) and any(cands[j] is not None for j in (AR, A, AL)) and n == 1
                seen["tie"] += bits[0] == bits[1] and lst[0][1] != lst[1][1]
                seen["own_cu"] += own
                seen["saturated"] += total > SAT
                seen["bits_33"] += max(eg(q[0] - lst[idx][1][0]), eg(q[1] - lst[idx][1][1])) == 33
                seen["priced"] += 1
    return out, mvp


OUTCOMES = ("num_spatial_0", "num_spatial_1", "num_spatial_2", "dedupe", "src_0", "src_1", "src_2", "src_3", "src_4", "src_5", "idx_1", "tie", "saturated", "bits_33")
# a square node has no candidate inside itself, and the 8x8 nodes' PUs are the small family's
APPLICABLE = {"nodes": OUTCOMES, "pu": OUTCOMES + ("own_cu",), "small": OUTCOMES + ("own_cu",)}
LEVELS = {"nodes": (0, 1, 2, 3), "pu": (0, 1, 2), "small": (2, 3)}


def same(got, exp, what=""):
    """every field of every record, of either record type"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype)
    for f in exp.dtype.names:
        bad = got[f] != exp[f]
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())


# ---- the random-record draw shared by the CPU tests and the GPU test -------------------------------------------------------------------------------

DRAW_W, DRAW_H = 168, 152          # 3 x 3 CTUs, a column 40 wide, a row 24 tall and the corner: a 64x64 node with a left, an above and a diagonal neighbour
DRAW_QP = 32
POOL = ((0, 0), (2, 2), (4, 4), (-5, 2), (3, 3), (32767, -32768), (-32768, 32767), (32767, 32767))


def random_records(rng, shape):
    """records of random bytes; vectors from POOL (so that equal neighbours and equal bit counts happen, and differences reach 33 bits per component),
    one record in ten marked, one satd_best in ten just below 2^32"""
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), QDT).reshape(shape).copy()
    pick = np.array(POOL, np.int16)[rng.integers(0, len(POOL), size=shape)]
    a["mvx"], a["mvy"] = pick[..., 0], pick[..., 1]
    a["cost_best"] = np.where(rng.random(shape) < 0.1, MARK, a["cost_best"] % 100000)
    a["satd_best"] = np.where(rng.random(shape) < 0.1, 0xFFFFFFF0 + rng.integers(0, 15, size=shape), a["satd_best"] % 50000).astype(np.uint32)
    return a


DRAWS = 60                         # tests/test_motion_amvp_ref.py asserts that this many show every applicable outcome, also on the four 64x64 nodes


def random_draw(seed, n_ctus=9):
    """(nodes [n_ctus, 85], pus [n_ctus, 124], small [n_ctus, 384]) of draw `seed`"""
    rng = np.random.default_rng(7000 + seed)
    return tuple(random_records(rng, (n_ctus, PER[f])) for f in ("nodes", "pu", "small"))


_BATCH = {}


def draw_batch():
    """all DRAWS as one batch of picture pairs at DRAW_QP, computed once: (inputs {family: [DRAWS, 9, per]}, expected {family: (records, predictor
    records)} alike, stats {family: {level: Counter}} summed over the draws)"""
    if not _BATCH:
        draws = [random_draw(s) for s in range(DRAWS)]
        stats = {}
        exp = [expected_all(DRAW_W, DRAW_H, *d, DRAW_QP, stats=stats) for d in draws]
        _BATCH["inputs"] = {f: np.stack([d[i] for d in draws]) for i, f in enumerate(("nodes", "pu", "small"))}
        _BATCH["expected"] = {f: (np.stack([e[f][0] for e in exp]), np.stack([e[f][1] for e in exp])) for f in PER}
        _BATCH["stats"] = stats
    return _BATCH["inputs"], _BATCH["expected"], _BATCH["stats"]


def expected_all(W, H, nodes, pus, small, qp, rows=None, stats=None):
    """all three families -> {family: (records, predictor records)}; stats: {family: {level: Counter}}"""
    out = {}
    for family, entries in (("nodes", nodes), ("pu", pus), ("small", small)):
        if entries is not None:
            out[family] = expected(W, H, nodes, entries, family, qp, rows, None if stats is None else stats.setdefault(family, {}))
    return out
