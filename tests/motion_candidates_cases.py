"""What the generator of tests/golden/ref_motion_candidates.npz (tests/quality/gen_motion_candidates_golden.py) and the two tests that read the file
(test_motion_candidates_pin.py without a GPU, test_gpu_motion_candidates_pin.py on the device) share: the picture and the draws of the file, the layout of a
recorded answer, the queries that ask the reference for it (record(): the generator and the regeneration test call it with oracle/_ref's library; nothing
else here needs it), the coverage counted from the reference's answers alone with the totals the file must show, and what a kernel must write, computed
from the file alone.  A plain module, not a conftest and not a test.

The reference's answers come from TComDataCU::fillMvpCand and TComDataCU::getInterMergeCandidates themselves, called by oracle/ref_rdo_harness.cpp
(href_mc_set_field / href_mc_query) on a motion field set by hand: for level l every CTU is tiled with 2Nx2N CUs of depth l, a CU inter with its node's
vector where the node is INSIDE and no marker, intra otherwise.  A node and the PUs of level l are queried on the field of level l: the same-level
neighbours the three stages define.  Not pinned by this file: the band rule (a band as a slice is not set up in the reference), neighbours of a finer
level, INSIDE (which the field expresses as intra by construction), and the tie departure from xCheckBestMVP."""
import collections
import os

import numpy as np

import motion_amvp_ref as ar
import motion_merge_ref as mg
import motion_refine_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_motion_candidates.npz")
W, H = ar.DRAW_W, ar.DRAW_H           # 168 x 152: 3 x 3 CTUs with a 40-wide column, a 24-tall row and the corner
CW, CH, N = 3, 3, 9
FAMILIES = ("nodes", "pu", "small")
PER = ar.PER
NAMES = ("L", "A", "AR", "BL", "AL")
L, A, AR, BL, AL = range(5)
SHAPES = ("2NxN", "Nx2N", "2NxnU", "2NxnD", "nLx2N", "nRx2N")
PART_SIZE = (1, 2, 4, 5, 6, 7)        # HM's PartSize of shape 0..5; 0 is SIZE_2Nx2N
MARK = ar.MARK
MERGE_RANGE = 8                       # its reach is 35 quarter samples
MERGE_POOL = ((0, 0), (2, 2), (-5, 2), (3, 3), (35, -35), (0, -7), (-35, 35))      # |component| <= 35: the reach condition excludes nothing
MARKER_RATE = 0.3
KINDS = ("amvp", "merge", "amvp", "merge", "amvp", "merge", "amvp", "merge")       # the draws of the file, in order
MERGE_DRAWS = tuple(d for d, k in enumerate(KINDS) if k == "merge")
AMVP_DRAWS = tuple(d for d, k in enumerate(KINDS) if k == "amvp")

# ---- the layout of one recorded answer: 40 int16 (oracle/ref_rdo_harness.cpp, href_mc_query) -------------------------------------------------------------
REC = 40
AMVP0, MERGE0, COUNT, FLAGS0 = 0, 4, 24, 25
#   [0..3]   the two AMVP candidates x0, y0, x1, y1
#   [4 + 4 i ..]  merge candidate i: mvx, mvy, inter direction, refIdx
#   [24]     numValidMergeCand + 16 * the number of spatial candidates in front of the zero fill
#   [25 + 3 j ..]  position j of L, A, AR, BL, AL: flags (bit 0: an inter neighbour with a vector; bit 1: it is the queried CU itself), mvx, mvy
# The merge part of an AMVP draw is stored as zeros: its vectors lie beyond every reach, where the merge stages have a stated departure.

# ---- the bit side ----------------------------------------------------------------------------------------------------------------------------------
DIFFS = sorted({0} | {s * v for k in range(17) for v in (1 << k, (1 << k) - 1) for s in (1, -1)} | {65535, -65535})


def bit_pairs():
    """[n, 4] int32 (vx, vy, px, py): every difference of DIFFS on each component against the zero predictor, and +-65535 as the two int16 extremes"""
    rows = [(d, 0, 0, 0) for d in DIFFS] + [(0, d, 0, 0) for d in DIFFS]
    rows += [(32767, 0, -32768, 0), (-32768, 0, 32767, 0), (0, 32767, 0, -32768), (0, -32768, 0, 32767), (32767, -32768, -32768, 32767)]
    return np.array(rows, np.int32)


def eg_array(v):
    """motion_amvp_ref.eg on an integer array: bit_length through frexp, exact for every int32"""
    v = np.asarray(v, np.int64)
    t = np.where(v <= 0, -2 * v + 1, 2 * v)
    return 2 * (np.frexp(t.astype(np.float64))[1].astype(np.int64) - 1) + 1


# ---- geometry of the entries -----------------------------------------------------------------------------------------------------------------------

def level_of(k):
    return mr.node_geometry(k)[0]


_TABLES = {}


def tables(family):
    """-> (covered entries [(k, s, p)], level per entry [per], INSIDE [N, per] bool, index of part 0 per entry [per] (itself for part 0 and nodes))"""
    if family not in _TABLES:
        cov = ar.covered(family)
        lvl = np.array([level_of(k) for k, _, _ in cov])
        ins = np.zeros((N, len(cov)), bool)
        for c in range(N):
            for e, (k, _, _) in enumerate(cov):
                l, bx, by = mr.node_geometry(k)
                ins[c, e] = mg.inside(W, H, l, (c % CW) * (1 << l) + bx, (c // CW) * (1 << l) + by)
        p0 = np.array([cov.index((k, s, 0)) if p == 1 else e for e, (k, s, p) in enumerate(cov)])
        _TABLES[family] = (cov, lvl, ins, p0)
    return _TABLES[family]


def compared(family, marker):
    """marker [..., N, per] -> bool alike: the entries a stage prices: INSIDE and no marker"""
    return tables(family)[2] & (marker == 0)


# ---- asking the reference (generator and regeneration test) ----------------------------------------------------------------------------------------------

def record(lib, mv, marker, with_merge):
    """mv {family: [N, per, 2] int16}, marker {family: [N, per] uint8} of ONE draw; lib: oracle_py.bind_candidates(load_ref()) -> {family: [N, per, REC]
    int16}: the reference's answer for every INSIDE entry, zeros elsewhere"""
    out = {f: np.zeros((N, PER[f], REC), np.int16) for f in FAMILIES}
    for lvl in range(4):
        first, n = mr.LEVEL_FIRST[lvl], 1 << lvl
        field_mv = np.ascontiguousarray(mv["nodes"][:, first:first + n * n], np.int16)
        field_inter = np.ascontiguousarray(marker["nodes"][:, first:first + n * n] == 0, np.uint8)
        assert lib.href_mc_set_field(W, H, lvl, field_mv, field_inter) == 0
        queries, where = [], []
        for f in FAMILIES:
            cov, levels, ins, p0 = tables(f)
            for e, (k, s, p) in enumerate(cov):
                if levels[e] != lvl:
                    continue
                for c in range(N):
                    if ins[c, e]:
                        set0 = int(p == 1 and marker[f][c, p0[e]] == 0)
                        v0 = mv[f][c, p0[e]] if set0 else (0, 0)
                        queries.append((c, k - first, 0 if s is None else PART_SIZE[s], p, set0, int(v0[0]), int(v0[1]), 0))
                        where.append((f, c, e))
        q = np.array(queries, np.int32)
        ans = np.zeros((len(queries), REC), np.int16)
        assert lib.href_mc_query(W, H, len(queries), q, ans) == len(queries)
        for (f, c, e), a in zip(where, ans):
            out[f][c, e] = a
    if not with_merge:
        for f in FAMILIES:
            out[f][..., MERGE0:COUNT + 1] = 0
    return out


def tables_from(lib):
    """-> (getCost [52, 67] uint32, bit counts [len(bit_pairs())] uint32)"""
    cost, pairs = np.zeros((52, 67), np.uint32), bit_pairs()
    bits = np.zeros(len(pairs), np.uint32)
    assert lib.href_mv_bit_tables(W, H, cost.reshape(-1), len(pairs), pairs.reshape(-1), bits) == 0
    return cost, bits


# ---- reading the file ------------------------------------------------------------------------------------------------------------------------------

_FILE = {}


def load():
    """-> the file's arrays: mv_<family> [D, N, per, 2] int16, marker_<family> [D, N, per] uint8, ref_<family> [D, N, per, REC] int16, kind [D] uint8
    (1 = merge draw), cost [52, 67], bit_pairs [n, 4], bit_counts [n]; read once"""
    if not _FILE:
        with np.load(GOLDEN) as z:
            _FILE.update({k: z[k] for k in z.files})
        assert [("amvp", "merge")[int(k)] for k in _FILE["kind"]] == list(KINDS)
    return _FILE


def draw(data, d):
    """-> (mv, marker, ref) {family: array} of draw d"""
    return tuple({f: data[f"{name}_{f}"][d] for f in FAMILIES} for name in ("mv", "marker", "ref"))


def flags(ref):
    """ref [..., REC] -> (found [..., 5] bool, own [..., 5] bool, vectors [..., 5, 2])"""
    fl = ref[..., FLAGS0:FLAGS0 + 15].reshape(ref.shape[:-1] + (5, 3))
    return (fl[..., 0] & 1) != 0, (fl[..., 0] & 2) != 0, fl[..., 1:]


def merge_list(ref):
    """-> (vectors [..., 5, 2], direction and refIdx [..., 5, 2], numValidMergeCand, number of spatial candidates)"""
    m = ref[..., MERGE0:MERGE0 + 20].reshape(ref.shape[:-1] + (5, 4))
    return m[..., :2], m[..., 2:], ref[..., COUNT] & 15, ref[..., COUNT] >> 4


# ---- coverage, counted from the reference's answers alone ------------------------------------------------------------------------------------------------

def coverage(data):
    """-> Counter: ("amvp", family, level, position) how often that position supplied an entry of the reference's AMVP list -- it is the first found of its
    group, (BL, L) or (AR, A, AL), and the list holds its vector in the group's slot --; ("own", shape) the same where the supplier is the queried CU
    itself; ("amvp_prune",) both groups found with equal vectors and the second slot a zero; ("merge_length", n) lists of n entries up to and including the
    first filled zero; ("al_dropped",) AL found, different from L and A where those are found, and not in a list of four spatial candidates;
    ("pair", a, b) a pruning pair found with equal vectors, neither being the queried CU itself.  All over the compared entries; the merge items over the
    merge draws."""
    seen = collections.Counter()
    for d, kind in enumerate(KINDS):
        mv, marker, ref = draw(data, d)
        for f in FAMILIES:
            cov, levels, _, _ = tables(f)
            found, own, vec = flags(ref[f])
            lists, _, _, spatial = merge_list(ref[f])
            for c, e in np.argwhere(compared(f, marker[f])):
                r, fd, vv = ref[f][c, e], found[c, e], vec[c, e]
                a = next((j for j in (BL, L) if fd[j]), None)
                b = next((j for j in (AR, A, AL) if fd[j]), None)
                pruned = a is not None and b is not None and tuple(vv[a]) == tuple(vv[b])
                slots = [j for j in (a, b) if j is not None][:1 if pruned else 2]
                for slot, j in enumerate(slots):
                    if tuple(r[2 * slot:2 * slot + 2]) == tuple(vv[j]):
                        seen[("amvp", f, int(levels[e]), NAMES[j])] += 1
                        if own[c, e, j]:
                            seen[("own", SHAPES[cov[e][1]])] += 1
                if pruned and tuple(r[2:4]) == (0, 0):
                    seen[("amvp_prune",)] += 1
                if kind != "merge":
                    continue
                seen[("merge_length", int(spatial[c, e]) + 1)] += 1
                differs = lambda x, y: not (fd[y] and not own[c, e, y] and tuple(vv[x]) == tuple(vv[y]))
                if fd[AL] and spatial[c, e] == 4 and differs(AL, L) and differs(AL, A) and tuple(vv[AL]) not in [tuple(v) for v in lists[c, e, :4]]:
                    seen[("al_dropped",)] += 1
                for x, y in ((A, L), (AR, A), (BL, L), (AL, L), (AL, A)):
                    if fd[x] and fd[y] and not own[c, e, x] and not own[c, e, y] and tuple(vv[x]) == tuple(vv[y]):
                        seen[("pair", NAMES[x], NAMES[y])] += 1
    return seen


MIN_SUPPLIED, MIN_SUPPLIED_ROOTS = 8, 4        # per family, level and position; on the four INSIDE 64x64 nodes
# combinations the geometry rules out; the reference must report zero for each
EXCUSED = {
    ("amvp", "nodes", 0, "BL"): "the CTU below-left of a 64x64 node follows it in coding order",
}


def required(family, level):
    return MIN_SUPPLIED_ROOTS if (family, level) == ("nodes", 0) else MIN_SUPPLIED


# ---- the totals of the file, from the generator's print-out ----------------------------------------------------------------------------------------------
COMPARED = {"nodes": 2920, "pu": 3636, "small": 12941}            # INSIDE entries that are no marker, all draws: what the AMVP stage prices
COMPARED_MERGE = {"nodes": 2052, "pu": 2592, "small": 9264}       # INSIDE entries of the merge draws: a merge list does not depend on the entry's own record
SUPPLIED = {                                                      # (family, level): how often L, A, AR, BL, AL supplied an entry of the AMVP list
    ("nodes", 0): (12, 8, 4, 0, 4),
    ("nodes", 1): (61, 41, 27, 21, 9),
    ("nodes", 2): (278, 157, 202, 82, 50),
    ("nodes", 3): (1179, 750, 866, 484, 223),
    ("pu", 0): (118, 79, 44, 35, 19),
    ("pu", 1): (557, 410, 358, 295, 60),
    ("pu", 2): (931, 614, 668, 442, 131),
    ("small", 2): (1811, 1255, 1329, 945, 271),
    ("small", 3): (3895, 2875, 3088, 2464, 685),
}
OWN = {"2NxN": 1791, "Nx2N": 2020, "2NxnU": 385, "2NxnD": 395, "nLx2N": 447, "nRx2N": 431}
MERGE_LENGTHS = {1: 1309, 2: 3519, 3: 2893, 4: 1568, 5: 390}
PAIRS = {("A", "L"): 327, ("AR", "A"): 1558, ("BL", "L"): 1448, ("AL", "L"): 1665, ("AL", "A"): 1678}
AL_DROPPED, AMVP_PRUNED = 21, 2125


# ---- what the stages must write, from the file alone -----------------------------------------------------------------------------------------------------

def records(rng, mv, marker):
    """refined records [..., per] MOTION_QPEL_DTYPE around stored vectors and marker flags: every other byte random, one satd_best in ten just below 2^32"""
    shape = marker.shape
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), ar.QDT).reshape(shape).copy()
    a["mvx"], a["mvy"] = mv[..., 0], mv[..., 1]
    a["cost_best"] = np.where(marker != 0, MARK, a["cost_best"] % 100000)
    a["satd_best"] = np.where(rng.random(shape) < 0.1, 0xFFFFFFF0 + rng.integers(0, 15, size=shape), a["satd_best"] % 50000).astype(np.uint32)
    return a


def amvp_expected(family, rec, ref, cost_row):
    """rec [..., N, per] input records, ref [..., N, per, REC], cost_row [67] = the reference's getCost at the QP -> (priced [..., N, per] bool, px, py, idx,
    bits, cost_best): the first index of least bits over the reference's two candidates"""
    priced = compared(family, rec["cost_best"] == MARK)
    q = np.stack([rec["mvx"], rec["mvy"]], -1).astype(np.int64)
    cand = ref[..., :4].reshape(ref.shape[:-1] + (2, 2)).astype(np.int64)
    bits = eg_array(q[..., None, 0] - cand[..., 0]) + eg_array(q[..., None, 1] - cand[..., 1])
    idx = (bits[..., 1] < bits[..., 0]).astype(np.int64)
    chosen = np.take_along_axis(bits, idx[..., None], -1)[..., 0]
    p = np.take_along_axis(cand, idx[..., None, None], -2)[..., 0, :]
    cost = np.minimum(rec["satd_best"].astype(np.int64) + np.asarray(cost_row, np.int64)[chosen], 0xFFFFFFFE)
    return priced, p[..., 0], p[..., 1], idx, chosen, cost


def check_amvp(family, rec, ref, cost_row, out, mvp, what=""):
    """the stage's two outputs for one family against amvp_expected -> how often index 1 won"""
    priced, px, py, idx, bits, cost = amvp_expected(family, rec, ref, cost_row)
    assert priced.any()
    for name, exp in (("px", px), ("py", py), ("idx", idx), ("bits", bits)):
        bad = priced & (mvp[name] != exp)
        assert not bad.any(), (what, family, name, int(bad.sum()), np.argwhere(bad)[:5].tolist(), mvp[name][bad][:5].tolist(), exp[bad][:5].tolist())
    bad = priced & (out["cost_best"] != cost)
    assert not bad.any(), (what, family, "cost_best", int(bad.sum()), np.argwhere(bad)[:5].tolist(), out["cost_best"][bad][:5].tolist(), cost[bad][:5].tolist())
    assert (mvp["idx"][~priced] == 255).all() and (out["cost_best"][~priced] == MARK).all(), (what, family, "entries that are not priced")
    return int(idx[priced].sum()), bits[priced]


def check_merge(family, ref, got, what=""):
    """merge records got [..., N, per] of one family against the reference's lists [..., N, per, REC]: every INSIDE entry has a valid record (the merge
    stages price marker entries too: a list does not depend on the entry's own record) -> the number of records compared"""
    ins = np.broadcast_to(tables(family)[2], got.shape)
    assert (got["num"][ins] > 0).all() and (got["cost_best"][~ins] == MARK).all(), (what, family)
    lists, _, _, spatial = merge_list(ref)
    idx = got["idx"].astype(np.int64)
    assert (idx[ins] <= spatial[ins]).all(), (what, family, "an index behind the first filled zero")
    v = np.take_along_axis(lists, np.minimum(idx, 4)[..., None, None], -2)[..., 0, :]
    for name, exp in (("mvx", v[..., 0]), ("mvy", v[..., 1]), ("num", spatial + 1)):
        bad = ins & (got[name] != exp)
        assert not bad.any(), (what, family, name, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[name][bad][:5].tolist(), exp[bad][:5].tolist())
    bad = ins & ((got["src"] == 5) != (idx == spatial))
    assert not bad.any(), (what, family, "src", int(bad.sum()), np.argwhere(bad)[:5].tolist())
    return int(ins.sum())
