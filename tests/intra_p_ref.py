"""Expected values of the intra stage of P pictures (fhevc_intra_p*) and of the tree decision that takes its costs (fhevc_p_tree_select_intra*), restated
in Python from the definitions in include/fasthevc.h -- not from the C code.  Python integers throughout (no 32-bit wrap can hide here).  The stage is a
pure function of the first-pass records; the tree is motion_skip_ref's skip tree with the two changed rules laid over it; real first-pass records come from
the CPU oracle (oracle_py), as tests/test_gpu_first_pass_4x4.py takes them; chain() runs one picture pair through the existing restatements of every
stage of fhevc_p_tree_intra_frame's zero-centred chain.  tests/test_intra_p_ref.py holds this module to hand-computed cases without a
GPU, tests/test_intra_p_abi.py compares the host twins with it, tests/test_gpu_intra_p.py the kernels.  A plain module, not a conftest and not a test."""
import math

import numpy as np

import motion_merge_ref as mg
import motion_skip_ref as sk
import p_tree_ref as pt
from fasthevc_amd import capi

MARK, SAT = 0xFFFFFFFF, 0xFFFFFFFE
IDT, NDT = capi.INTRA_P_DTYPE, capi.NODE_DTYPE
INTRA = 1                                     # bit 0 of byte 14 (pad[0]) of a tree record
MARKER = (MARK, MARK, (255, 255, 255, 255), 0, (0, 0, 0))
DRAW_QP = 32                                  # the QP the draw's NxN cases are built around (any QP is legal on it)
DRAW_PICTURES = 14                         # see test_intra_p_ref.test_the_draw_shows_every_case
DRAW_SIZES = ((200, 136), (100, 76))


# ---- the stage ----------------------------------------------------------------------------------------------------------------------------------------

def bits(m):
    """the first pass's model of a mode's bits, on a byte value"""
    return 2 if m == 0 else (3 if m in (1, 26) else 6)


def sqrt_lambda(qp):
    return math.sqrt(0.57 * math.pow(2.0, (qp - 12.0) / 3.0))


def bit_costs(qp):
    """c[b] for b in {2, 3, 6}: getCost(b) = (uint32_t)((motion_lambda * b) / 65536.0), motion_lambda = 65536 sqrt(lambda), in doubles"""
    ml = 65536.0 * sqrt_lambda(qp)
    return {b: int((ml * b) / 65536.0) for b in (2, 3, 6)}


def price(satd, mode, c):
    """of a priced record (satd != MARK); mode: the record's mode dword, of which the low byte counts"""
    return min(int(satd) + c[bits(int(mode) & 255)], SAT)


def node_record(k, valid_w, valid_h, first, first4, c):
    """first: the CTU's 85 (satd, mode) pairs; first4: its 256 pairs or None -> the record tuple of node k"""
    inside = pt.geometry(k, valid_w, valid_h)[0]
    if not inside:
        return MARKER
    satd, mode = int(first[k][0]), int(first[k][1]) & 255
    best = (satd, price(satd, mode, c), (mode,) * 4, 0, (0, 0, 0)) if satd != MARK else None
    l, x, y = pt.node_pos(k)
    if l == 3 and first4 is not None:
        pus = [first4[(2 * y + dy) * 16 + 2 * x + dx] for dy in (0, 1) for dx in (0, 1)]
        if all(int(s) != MARK for s, _ in pus):
            cost4 = min(sum(price(s, m, c) for s, m in pus), SAT)
            if best is None or cost4 < best[1]:
                best = (min(sum(int(s) for s, _ in pus), SAT), cost4, tuple(int(m) & 255 for _, m in pus), 1, (0, 0, 0))
    return best if best is not None else MARKER


def stage(first, first4, W, H, qp, rows=None):
    """first [P, band CTUs, 85], first4 [P, band CTUs, 256] or None: NODE_DTYPE records compact over CTU rows `rows` of a W x H picture -> [P, band CTUs, 85] IDT"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rb, re = rows if rows is not None else (0, ch)
    P, nb = first.shape[:2]
    assert nb == (re - rb) * cw and (first4 is None or first4.shape == (P, nb, 256))
    c = bit_costs(qp)
    out = np.zeros((P, nb, 85), IDT)
    for p in range(P):
        for i in range(nb):
            vw, vh = pt.valid_size(rb * cw + i, W, H)
            f = list(zip(first["satd"][p, i].tolist(), first["mode"][p, i].tolist()))
            f4 = list(zip(first4["satd"][p, i].tolist(), first4["mode"][p, i].tolist())) if first4 is not None else None
            for k in range(85):
                out[p, i, k] = node_record(k, vw, vh, f, f4, c)
    return out


def same(got, exp, what=""):
    """every byte of every record"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    for f in IDT.names:
        bad = got[f] != exp[f]
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())


# ---- the tree decision with the intra candidate: the skip tree with two changed rules ---------------------------------------------------------------

def tree_ctu(shape_cost, merge_cost, skip_flags, skip_mask, intra_cost, valid_w, valid_h, rule=None):
    """one CTU -> (records [85] TREE_DTYPE, depth_min, depth_max [256]).  An INSIDE node of any level that is not calm (merge cost strictly smaller AND a masked
    zero bit) and whose intra cost is strictly below inter = min(selection, merge) takes the intra cost as its own: that is the skip tree on a selection cost
    replaced by the intra cost -- the replaced node is then neither merged nor stopped early there, as the definition wants it --, with bit 6 restored from the
    original costs and bit 0 of byte 14 set."""
    sc = [int(v) for v in shape_cost]
    taken, merged = [False] * 85, [False] * 85
    for k in range(85):
        if not pt.geometry(k, valid_w, valid_h)[0]:
            continue
        mc, ic = int(merge_cost[k]), int(intra_cost[k])
        merged[k] = mc < sc[k]
        calm = merged[k] and (int(skip_flags[k]) & skip_mask) != 0
        taken[k] = not calm and ic < min(sc[k], mc)
    rec, dmin, dmax = sk.tree_ctu([int(intra_cost[k]) if taken[k] else sc[k] for k in range(85)], merge_cost, skip_flags, skip_mask, valid_w, valid_h, rule)
    for k in range(85):
        if taken[k]:
            assert not rec["flags"][k] & (mg.MERGED | sk.SKIPPED) and int(rec["cost_own"][k]) == int(intra_cost[k])
            rec["flags"][k] |= mg.MERGED if merged[k] else 0
            rec["pad"][k, 0] = INTRA
    return rec, dmin, dmax


def tree_select(shapes, merge, skip, skip_mask, intra, W, H, rows=None, rule=None):
    """shapes / merge / skip / intra: [P, band CTUs, 85] records -> (records, depth_min, depth_max) as p_tree_ref.select"""
    sc, mc, sf, ic = shapes["cost_best"], merge["cost_best"], skip["flags"], intra["cost_best"]
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rb, re = rows if rows is not None else (0, ch)
    P, nb = sc.shape[:2]
    assert nb == (re - rb) * cw
    rec, dmin, dmax = np.zeros((P, nb, 85), pt.TDT), np.zeros((P, nb, 256), np.uint8), np.zeros((P, nb, 256), np.uint8)
    for p in range(P):
        for i in range(nb):
            rec[p, i], dmin[p, i], dmax[p, i] = tree_ctu(sc[p, i], mc[p, i], sf[p, i], skip_mask, ic[p, i], *pt.valid_size(rb * cw + i, W, H), rule)
    return rec, dmin, dmax


def same_tree(got, exp, what=""):
    """every byte of every tree record, byte 14 included"""
    pt.same(got, exp, what)
    assert got.tobytes() == exp.tobytes(), (what, "pad", np.argwhere(got["pad"] != exp["pad"])[:5].tolist())


# ---- the draw: random records that make every case of both definitions occur (shared by the CPU, ABI and GPU tests) ---------------------------------------

STAGE_CASES = ("priced", "unpriced", "not_inside")                       # at every level 0..3
NXN_CASES = ("nxn_one_less", "nxn_tie", "nxn_one_more", "pu_unpriced", "only_nxn", "neither", "price_saturated", "sum_saturated")   # at level 3
TREE_CASES = ("intra_one_less", "intra_equal", "intra_one_more", "calm_withheld", "mark_intra")                                       # at every level 0..3


def random_first(rng, P, n, qp=DRAW_QP):
    """(first [P, n, 85], first4 [P, n, 256]) NODE_DTYPE: every byte random -- the double and the high bytes of mode must not matter --, then satd and the low
    byte of mode set per record: modes from {0, 1, 26, 10, 34, 35, 200, 255}; satd small, MARK one time in eight, near 2^32 one time in sixteen; and per 8x8
    node, half of the time, the node's satd chosen so that its price lies 1 below, on, or 1 above the NxN cost of its four PUs"""
    c = bit_costs(qp)
    modes = np.array([0, 1, 26, 10, 34, 35, 200, 255], np.uint32)

    def records(count):
        a = np.frombuffer(rng.bytes(P * n * count * 16), NDT).reshape(P, n, count).copy()
        a["mode"] = (a["mode"] & 0xFFFFFF00) | rng.choice(modes, size=(P, n, count))
        satd = rng.integers(0, 3000, size=(P, n, count)).astype(np.uint32)
        u = rng.random((P, n, count))
        satd = np.where(u < 1 / 16, rng.choice(np.array([SAT, SAT - 1, SAT - 5, 0xFFFFFFF0, 0x7FFFFFFF, 0x80000000], np.uint32), size=(P, n, count)), satd)
        a["satd"] = np.where((u >= 1 / 16) & (u < 3 / 16), MARK, satd)
        return a

    first, first4 = records(85), records(256)
    for p in range(P):
        for i in range(n):
            for k in range(21, 85):
                if rng.random() < 0.5:
                    continue
                _, x, y = pt.node_pos(k)
                pus = [first4[p, i, (2 * y + dy) * 16 + 2 * x + dx] for dy in (0, 1) for dx in (0, 1)]
                if any(int(q["satd"]) == MARK for q in pus):
                    continue
                want = min(sum(price(q["satd"], q["mode"], c) for q in pus), SAT) + int(rng.integers(-1, 2)) - c[bits(int(first["mode"][p, i, k]) & 255)]
                if 0 <= want < SAT:
                    first["satd"][p, i, k] = want
    return first, first4


def stage_coverage(first, first4, out, W, H, qp, rows=None, seen=None):
    """how often each case of the stage's definition occurs, per level -> {(case, level): count}"""
    seen = seen if seen is not None else {}
    c = bit_costs(qp)
    cw = (W + 63) // 64
    rb = rows[0] if rows is not None else 0

    def hit(case, l):
        seen[(case, l)] = seen.get((case, l), 0) + 1

    for p in range(first.shape[0]):
        for i in range(first.shape[1]):
            vw, vh = pt.valid_size(rb * cw + i, W, H)
            for k in range(85):
                l, x, y = pt.node_pos(k)
                if not pt.geometry(k, vw, vh)[0]:
                    hit("not_inside", l)
                    continue
                satd = int(first["satd"][p, i, k])
                hit("priced" if satd != MARK else "unpriced", l)
                if l < 3:
                    continue
                pus = [first4[p, i, (2 * y + dy) * 16 + 2 * x + dx] for dy in (0, 1) for dx in (0, 1)]
                have4 = all(int(q["satd"]) != MARK for q in pus)
                if not have4:
                    hit("pu_unpriced" if satd != MARK and sum(int(q["satd"]) == MARK for q in pus) == 1 else "neither" if satd == MARK else "pu_unpriced_more", l)
                    continue
                total = sum(price(q["satd"], q["mode"], c) for q in pus)
                if total > SAT:
                    hit("sum_saturated", l)
                if satd == MARK:
                    hit("only_nxn", l)
                    continue
                if satd + c[bits(int(first["mode"][p, i, k]) & 255)] > SAT:
                    hit("price_saturated", l)
                d = min(total, SAT) - price(satd, first["mode"][p, i, k], c)
                if d in (-1, 0, 1):
                    hit(("nxn_one_less", "nxn_tie", "nxn_one_more")[d + 1], l)
                    assert int(out["part"][p, i, k]) == (1 if d < 0 else 0)
    return seen


def random_tree_inputs(rng, P, n):
    """(shapes, merge, skip, intra) [P, n, 85]: the skip tree's draw (p_tree_ref.random_shapes, motion_merge_ref.random_merge, motion_skip_ref.random_skip) and intra
    records of random bytes whose cost_best lies 1 below, on, 1 above or well off the node's inter cost, or is MARK (one time in six); where both inter costs
    are MARK the intra cost is a small number or MARK"""
    shapes = pt.random_shapes(rng, P, n)
    merge = mg.random_merge(rng, shapes)
    skip = sk.random_skip(rng, (P, n, 85))
    intra = np.frombuffer(rng.bytes(P * n * 85 * 16), IDT).reshape(P, n, 85).copy()
    inter = np.minimum(shapes["cost_best"], merge["cost_best"]).astype(np.int64)
    base = np.where(inter == MARK, rng.integers(50, 5000, size=inter.shape), inter)
    c = np.clip(base + rng.choice([-40, -1, -1, 0, 0, 1, 1, 40], size=inter.shape), 0, SAT)
    intra["cost_best"] = np.where(rng.random(inter.shape) < 1 / 6, MARK, c).astype(np.uint32)
    return shapes, merge, skip, intra


def tree_coverage(shapes, merge, skip, intra, skip_mask, rec, W, H, rows=None, seen=None):
    """how often each case of the two changed rules occurs, per level -> {(case, level): count}; checks the intra bit against the case on the way"""
    seen = seen if seen is not None else {}
    cw = (W + 63) // 64
    rb = rows[0] if rows is not None else 0
    for p in range(shapes.shape[0]):
        for i in range(shapes.shape[1]):
            vw, vh = pt.valid_size(rb * cw + i, W, H)
            for k in range(85):
                if not pt.geometry(k, vw, vh)[0]:
                    continue
                l = pt.level(k)
                sc, mc, ic = int(shapes["cost_best"][p, i, k]), int(merge["cost_best"][p, i, k]), int(intra["cost_best"][p, i, k])
                inter, calm = min(sc, mc), mc < sc and (int(skip["flags"][p, i, k]) & skip_mask) != 0
                bit = bool(rec["pad"][p, i, k, 0] & INTRA)
                case = None
                if ic == MARK:
                    case = "mark_intra"
                elif calm and ic < inter:
                    case = "calm_withheld"
                elif not calm and inter != MARK and ic - inter in (-1, 0, 1):
                    case = ("intra_one_less", "intra_equal", "intra_one_more")[ic - inter + 1]
                assert bit == (not calm and ic < inter), (p, i, k)
                if case:
                    seen[(case, l)] = seen.get((case, l), 0) + 1
    return seen


_DRAW = {}


def draw(size):
    """the draw on a W x H picture of DRAW_SIZES, DRAW_PICTURES pictures: dict(first, first4, out, out_no4 -- the stage's expectation with and without the 4x4
    records at DRAW_QP --, shapes, merge, skip, intra, rules, tree: {(rule name, mask): (records, depth_min, depth_max)}); computed once, never changed"""
    if size not in _DRAW:
        W, H = size
        n = ((W + 63) // 64) * ((H + 63) // 64)
        rng = np.random.default_rng(823 + W)
        first, first4 = random_first(rng, DRAW_PICTURES, n)
        shapes, merge, skip, intra = random_tree_inputs(rng, DRAW_PICTURES, n)
        rules = {"default": capi.p_tree_rule_default(), "r1": pt.random_rule(rng), "r2": pt.random_rule(rng), "r3": pt.random_rule(rng)}
        _DRAW[size] = dict(first=first, first4=first4, out=stage(first, first4, W, H, DRAW_QP), out_no4=stage(first, None, W, H, DRAW_QP), shapes=shapes, merge=merge,
                           skip=skip, intra=intra, rules=rules, tree={})
    return _DRAW[size]


def draw_tree(size, rule_name, mask):
    d = draw(size)
    if (rule_name, mask) not in d["tree"]:
        d["tree"][(rule_name, mask)] = tree_select(d["shapes"], d["merge"], d["skip"], mask, d["intra"], *size, rule=d["rules"][rule_name])
    return d["tree"][(rule_name, mask)]


def all_mark(intra):
    a = intra.copy()
    a["cost_best"] = MARK
    return a


# ---- real records: the CPU oracle's two first passes of a picture -----------------------------------------------------------------------------------------------

def oracle_first_passes(oracle, op, pic, bd, qp):
    """pic [H, W] samples -> (first [numCtus, 85], first4 [numCtus, 256]) NODE_DTYPE, from the oracle's fho_first_pass_ctu and, through
    first_pass_4x4_ref.expected, its fho_first_pass_node at n = 4"""
    import first_pass_4x4_ref as f4
    H, W = pic.shape
    cw, ch = (W + 63) // 64, (H + 63) // 64
    flat = np.ascontiguousarray(pic.astype(np.int16)).reshape(-1)
    sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
    first = np.zeros((cw * ch, 85), NDT)
    e85 = (op.NodeCost * 85)()
    for c in range(cw * ch):
        oracle.fho_first_pass_ctu(op.ptr(flat, 0), W, W, H, c % cw, c // cw, bd, sl, e85)
        first[c] = np.frombuffer(e85, dtype=NDT)
    return first, f4.expected(oracle, flat, 0, W, W, H, bd, qp)["best"]


# ---- the constructed pair: a flat CTU beside a CTU that is the reference displaced by half a sample --------------------------------------------------------------

PAIR_W, PAIR_H, PAIR_QP = 128, 64, 32


def constructed_pair(bd):
    """(cur, ref) [64, 128] int64: the reference is noise; CTU 0 of the current picture is flat at 1 << (bd - 1), CTU 1 is the reference displaced by half a
    sample to the left through HEVC's 8-tap filter itself (coordinates clamped to the picture)"""
    import motion_refine_ref as mr
    rng = np.random.default_rng(4100 + bd)
    ref = rng.integers(0, 1 << bd, size=(PAIR_H, PAIR_W)).astype(np.int64)
    cur = np.full((PAIR_H, PAIR_W), 1 << (bd - 1), np.int64)
    cur[:, 64:] = mr.Planes(ref, bd, 16).block(2, 0, 64, 0, 64)
    return cur, ref


# ---- the chain of fhevc_p_tree_intra_frame (coarse_range 0), from the existing restatements and the oracle's first passes ---------------------------------------

CHAIN_RANGE = 8
_CHAIN = {}


def chain_records(oracle, op, cur, ref, bd, qp, search_range=CHAIN_RANGE):
    """cur / ref [H, W] samples -> dict of the [numCtus, 85] records the tree reads: shapes, merge, skip, intra.  The stages in the frame chain's order: SAD search of the three families (motion_range_sweep), quarter-sample
    refinement (motion_refine_ref, motion_refine_pu_ref), re-pricing against neighbour predictors (motion_amvp_ref), merge per node and per PU on the
    re-priced records (motion_merge_ref, motion_merge_pu_ref), merge-aware selection (motion_merge_pu_ref.select), the zero-residual stage on the node merge
    records (motion_skip_ref), the oracle's two first passes of the current picture and the intra stage of this module"""
    import motion_amvp_ref as am
    import motion_merge_pu_ref as mpr
    import motion_range_sweep as sw
    import motion_refine_pu_ref as rp
    import motion_refine_ref as mr
    H, W = cur.shape
    R = search_range
    cur, ref = cur.astype(np.int64), ref.astype(np.int64)
    found = sw.PairSweep(oracle, cur, ref, bd, qp, sad=True, rmax=R).records(R)
    cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
    planes = mr.Planes(ref, bd, R + 8)
    nodes = mr.expected(oracle, cur_flat, 0, W, ref, W, H, bd, qp, found["nodes"], R, planes=planes)
    pu = rp.expected(oracle, cur, ref, bd, qp, found["pu"], R, "pu", planes=planes)
    small = rp.expected(oracle, cur, ref, bd, qp, found["small"], R, "small", planes=planes)
    priced = {f: v[0] for f, v in am.expected_all(W, H, nodes, pu, small, qp).items()}
    merge = mg.expected(oracle, cur_flat, 0, W, ref, W, H, bd, qp, priced["nodes"], R, planes=planes)
    mpu, msmall = (mpr.expected(oracle, cur_flat, 0, W, ref, W, H, bd, qp, priced["nodes"], R, f, planes=planes) for f in ("pu", "small"))
    shapes = mpr.select(priced["nodes"][None], priced["pu"][None], priced["small"][None], mpu[None], msmall[None], W, H)[0][0]
    skip = sk.expected(cur, ref, W, H, bd, qp, merge, R, planes=planes)
    first, first4 = oracle_first_passes(oracle, op, cur, bd, qp)
    return dict(shapes=shapes, merge=merge, skip=skip, intra=stage(first[None], first4[None], W, H, qp)[0])


def chain(oracle, op, cur, ref, bd, qp, skip_mask, search_range=CHAIN_RANGE, tree_rule=None):
    """chain_records and the two trees on them -> dict of [numCtus, ...] arrays: shapes, merge, skip, intra, tree, dmin, dmax (the tree of this module), and
    skip_tree / skip_dmin / skip_dmax (the tree that stops at a skip on the same records)"""
    H, W = cur.shape
    r = chain_records(oracle, op, cur, ref, bd, qp, search_range)
    shapes, merge, skip, intra = r["shapes"], r["merge"], r["skip"], r["intra"]
    tree, dmin, dmax = (a[0] for a in tree_select(shapes[None], merge[None], skip[None], skip_mask, intra[None], W, H, rule=tree_rule))
    s_tree, s_min, s_max = (a[0] for a in sk.tree_select(shapes[None], merge[None], skip[None], skip_mask, W, H, rule=tree_rule))
    return dict(shapes=shapes, merge=merge, skip=skip, intra=intra, tree=tree, dmin=dmin, dmax=dmax, skip_tree=s_tree, skip_dmin=s_min, skip_dmax=s_max)


def constructed_chain(oracle, op, bd, skip_mask=3):
    """the constructed pair through chain() at PAIR_QP; computed once per bit depth and mask"""
    if (bd, skip_mask) not in _CHAIN:
        _CHAIN[(bd, skip_mask)] = chain(oracle, op, *constructed_pair(bd), bd, PAIR_QP, skip_mask)
    return _CHAIN[(bd, skip_mask)]


def check_constructed(got, c2):
    """what the constructed pair must show, on a dict with tree [2, 85], dmin / dmax [2, 256], intra [2, 85] and skip_dmin / skip_dmax [2, 256]: CTU 0 -- every
    intra record satd 0, mode 0, cost c[2]; the root's cost_tree == c[2] with the intra bit; both maps 0 everywhere.  CTU 1 -- no node carries the intra bit,
    and the maps are the skip tree's"""
    i0 = got["intra"][0]
    assert (i0["satd_best"] == 0).all() and (i0["cost_best"] == c2).all() and (i0["modes"] == 0).all() and (i0["part"] == 0).all()
    assert int(got["tree"]["cost_tree"][0, 0]) == c2 and got["tree"]["pad"][0, 0, 0] == INTRA
    assert not got["dmin"][0].any() and not got["dmax"][0].any()
    assert not got["tree"]["pad"][1].any(), np.flatnonzero(got["tree"]["pad"][1, :, 0])
    assert np.array_equal(got["dmin"][1], got["skip_dmin"][1]) and np.array_equal(got["dmax"][1], got["skip_dmax"][1])
