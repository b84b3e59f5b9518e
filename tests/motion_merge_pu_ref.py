"""Expected values of the merge stage per PU (fhevc_motion_merge_pu*) and of the partition-size selection that takes its costs
(fhevc_pu_shape_select_merge*), restated in Python from the definitions in include/fasthevc.h -- not from the C code: a PU's rectangle, its five candidate
samples, the same-level nodes that hold them and their availability; the list and the choice are motion_merge_ref's (build_list, choose), the distortion
of a w x h block at a quarter-sample vector the CPU oracle's fho_satd on motion_refine_ref.Planes, the selection's one rule sits on pu_shape_ref.
tests/test_motion_merge_pu_ref.py pins this module without a GPU, tests/test_motion_merge_pu_abi.py compares the host functions with it,
tests/test_gpu_motion_merge_pu.py the kernels.  A plain module, not a conftest and not a test."""
import ctypes as C

import numpy as np

import motion_merge_ref as mg
import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_refine_ref as mr
import pu_shape_ref as sr
from fasthevc_amd import capi

MARK = mg.MARK
MDT, QDT = capi.MOTION_MERGE_DTYPE, capi.MOTION_QPEL_DTYPE
FAMILIES = {"pu": (mp.covered, 124), "small": (ps.covered, 384)}
NAMES = ("L", "A", "AR", "BL", "AL")


def samples(x, y, w, h):
    """HM's five candidate samples of the PU (x, y, w, h): L, A, AR, BL, AL"""
    return ((x - 1, y + h - 1), (x + w - 1, y - 1), (x + w, y - 1), (x - 1, y + h), (x - 1, y - 1))


def pu_geometry(W, c, k, s, p):
    """PU (shape s, part p) of CU node k of CTU c (raster) of a picture W samples wide -> (level, (gx, gy) of the CU on its level's grid, the PU's rectangle
    (x, y, w, h) in picture samples)"""
    cw = (W + 63) // 64
    lvl, bx, by = mr.node_geometry(k)
    x0, y0, w, h = mp.pu_rect(k, s, p)
    return lvl, ((c % cw) * (1 << lvl) + bx, (c // cw) * (1 << lvl) + by), ((c % cw) * 64 + x0, (c // cw) * 64 + y0, w, h)


def candidates(W, H, rows, c, k, s, p):
    """the five candidate positions of a PU -> per position None, or (ctu raster index, node index) of the node of the CU's own level that holds the sample,
    if it lies on the grid, is INSIDE, belongs to a CTU row of the band `rows` and its coding-order key is strictly smaller than that of the PU's own CU"""
    cw = (W + 63) // 64
    lvl, (gx, gy), rect = pu_geometry(W, c, k, s, p)
    size, n = 64 >> lvl, 1 << lvl
    own = mg.key(cw, lvl, gx, gy)
    out = []
    for sx, sy in samples(*rect):
        if sx < 0 or sy < 0:
            out.append(None)
            continue
        x, y = sx // size, sy // size
        ok = mg.inside(W, H, lvl, x, y) and rows[0] <= (y >> lvl) < rows[1] and mg.key(cw, lvl, x, y) < own
        out.append(((y >> lvl) * cw + (x >> lvl), mg.node_index(lvl, x & (n - 1), y & (n - 1))) if ok else None)
    return out


def satd_block(oracle, planes, cur_flat, origin, stride, x, y, w, h, q):
    """xGetHADs of the w x h block at (x, y) against the reference displaced by q = (qx, qy) quarter samples: fho_satd takes xGetHADs' own branch"""
    cur = C.c_void_p(cur_flat.ctypes.data + 2 * (origin + y * stride + x))
    return int(oracle.fho_satd(cur, stride, planes.block_ptr(q[0], q[1], x, y), planes.width, w, h, planes.bd))


def pu_lists(W, H, rows, refined, max_range, family):
    """refined [band CTUs, 85] -> per band CTU and entry of the family None (the PU's CU node is not INSIDE) or (rectangle, the five candidates as
    build_list takes them, the list)"""
    cw = (W + 63) // 64
    cov = FAMILIES[family][0]()
    out = []
    for i in range(refined.shape[0]):
        c = rows[0] * cw + i
        per = []
        for k, s, p in cov:
            lvl, (gx, gy), rect = pu_geometry(W, c, k, s, p)
            if not mg.inside(W, H, lvl, gx, gy):
                per.append(None)
                continue
            cands = []
            for nb in candidates(W, H, rows, c, k, s, p):
                r = None if nb is None else refined[nb[0] - rows[0] * cw, nb[1]]
                cands.append(None if r is None else (int(r["cost_best"]), int(r["mvx"]), int(r["mvy"])))
            per.append((rect, cands, mg.build_list(cands, max_range)))
        out.append(per)
    return out


def expected(oracle, cur_flat, origin, stride, ref_pic, W, H, bd, qp, refined, max_range, family, rows=None, planes=None):
    """refined: [band CTUs, 85] MOTION_QPEL_DTYPE (cost_best, mvx, mvy are read), compact over the CTU rows `rows` (default: the whole picture)
    -> [band CTUs, 124 or 384] MOTION_MERGE_DTYPE of family "pu" or "small\""""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rows = rows if rows is not None else (0, ch)
    nb = (rows[1] - rows[0]) * cw
    refined = refined.reshape(nb, 85)
    planes = planes or mr.Planes(ref_pic, bd, max_range + 8)
    assert planes.pad >= max_range + 6 and planes.bd == bd
    sl = mr.sqrt_lambda(oracle, qp, bd)
    out = np.zeros((nb, FAMILIES[family][1]), MDT)
    for i, per in enumerate(pu_lists(W, H, rows, refined, max_range, family)):
        for e, item in enumerate(per):
            if item is None:
                out[i, e] = mg.INVALID
                continue
            (x, y, w, h), _, entries = item
            satds = [satd_block(oracle, planes, cur_flat, origin, stride, x, y, w, h, q) for _, q in entries]
            out[i, e] = mg.choose(entries, satds, sl)
    return out


def list_statistics(W, H, rows, refined, max_range, family):
    """what the lists of one picture's refined records [band CTUs, 85] show for a family: the set of lengths, and per pruning pair how often it fired (both
    available, equal vectors) and how often it did not (both available, different vectors)"""
    reach = 4 * max_range + 3
    lengths = set()
    pairs = {n: [0, 0] for n in ("A_L", "AR_A", "BL_L", "AL_L", "AL_A")}
    for per in pu_lists(W, H, rows, refined, max_range, family):
        for item in per:
            if item is None:
                continue
            _, cands, lst = item
            v = [None if c is None or c[0] == MARK or abs(c[1]) > reach or abs(c[2]) > reach else c[1:] for c in cands]
            lengths.add(len(lst))
            for name, a, b in (("A_L", 1, 0), ("AR_A", 2, 1), ("BL_L", 3, 0), ("AL_L", 4, 0), ("AL_A", 4, 1)):
                if v[a] is not None and v[b] is not None:
                    pairs[name][0 if v[a] == v[b] else 1] += 1
    return lengths, pairs


def same(got, exp, what=""):
    mg.same(got, exp, what)


# ---- the random-record draw shared by the CPU test and the GPU test -------------------------------------------------------------------------------

DRAW_W, DRAW_H, DRAW_QP, DRAW_RANGE = 200, 136, 4, 8      # 4 x 3 CTUs, ragged by 8 both ways; bits are cheap at qp 4: any list position can win


def random_refined(rng, shape, max_range, pool=None):
    """refined records of random bytes; vectors drawn from four near ones (so that every pruning pair fires), one record in ten out of reach (one quarter
    sample beyond it, or anywhere), one in seven marked; pool: other vectors to draw from, in their place (tests/motion_merge_sweep_cases.py)"""
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), QDT).reshape(shape).copy()
    reach = 4 * max_range + 3
    pool = np.array([(-5, 2), (3, 3), (reach, -reach), (0, -7)] if pool is None else pool, np.int16)
    pick = pool[rng.integers(0, len(pool), size=shape)]
    far = rng.random(shape) < 0.1
    beyond = np.where(rng.random(shape) < 0.5, reach + 1, rng.integers(reach + 1, 32768, size=shape)) * rng.choice([-1, 1], size=shape)
    a["mvx"] = np.where(far & (rng.random(shape) < 0.5), beyond, pick[..., 0])
    a["mvy"] = np.where(far & (a["mvx"] == pick[..., 0]), beyond, pick[..., 1])
    a["cost_best"] = np.where(rng.random(shape) < 1 / 7, MARK, a["cost_best"] % 100000)
    return a


def random_draw():
    """(pictures [2][H, W] int64 noise at 8 bit, refined [12, 85]) of the draw"""
    rng = np.random.default_rng(2024)
    pics = [rng.integers(0, 256, size=(DRAW_H, DRAW_W)).astype(np.int64) for _ in range(2)]
    return pics, random_refined(np.random.default_rng(77), (12, 85), DRAW_RANGE)


def check_draw(refined, exp, family):
    """the draw holds every list length, every source as a winner and every pruning pair both ways"""
    lengths, pairs = list_statistics(DRAW_W, DRAW_H, (0, 3), refined, DRAW_RANGE, family)
    assert lengths == {1, 2, 3, 4, 5}, (family, lengths)
    assert all(f > 0 and n > 0 for f, n in pairs.values()), (family, pairs)
    ok = exp["num"] > 0
    assert set(np.unique(exp["src"][ok])) == {0, 1, 2, 3, 4, 5} and set(np.unique(exp["num"][ok])) == {1, 2, 3, 4, 5}, (family, np.unique(exp["src"][ok]))
    assert ok.any() and not ok.all()


# ---- the selection's one rule on top of pu_shape_ref ------------------------------------------------------------------------------------------------

def _cost(a):
    return None if a is None else (a["cost_best"] if a.dtype.names else a).astype(np.uint32)


def select(nodes, pus, pus_small, merge_pus, merge_small, W, H, rows=None, rule=None):
    """pu_shape_ref.select with the merge records [P, band CTUs, 124] / [P, band CTUs, 384] (or None: all markers, as a None pus_small) beside the refined
    entries: a part costs the smaller of its refined and its merge cost_best, the marker being the largest value
    -> (records, costs, merged [P, band CTUs, 85] uint16: bit 2 p + part set iff that part's merge cost is strictly smaller than its refined cost)"""
    pc, sc, mpc, msc = _cost(pus), _cost(pus_small), _cost(merge_pus), _cost(merge_small)
    fill = lambda a, like, n: np.full(like.shape[:2] + (n,), MARK, np.uint32) if a is None else a
    small_any = sc is not None or msc is not None
    sc, msc = fill(sc, pc, 384), fill(msc, pc, 384)
    rec, costs = sr.select(_cost(nodes), np.minimum(pc, mpc), np.minimum(sc, msc) if small_any else None, W, H, rows=rows, rule=rule)
    cw = (W + 63) // 64
    rb = rows[0] if rows is not None else 0
    merged = np.zeros(rec.shape, np.uint16)
    for i in range(rec.shape[1]):
        ctu = rb * cw + i
        vw, vh = min(64, W - (ctu % cw) * 64), min(64, H - (ctu // cw) * 64)
        for k in range(85):
            x, y, n = sr.node_rect(k)
            if x + n > vw or y + n > vh:
                continue
            for p in (1, 2, 4, 5, 6, 7):
                w = sr.parts(k, p)
                if w is None:
                    continue
                ref_, mrg = (pc, mpc) if w[0] == "pu" else (sc, msc)
                for part in (0, 1):
                    merged[:, i, k] |= np.where(mrg[:, i, w[1 + part]] < ref_[:, i, w[1 + part]], 1 << (2 * p + part), 0).astype(np.uint16)
    return rec, costs, merged


def random_pu_merge(rng, pus, pus_small):
    """merge records beside pu_shape_ref.random_entries' PUs: cost_best a hair around the refined entry's, equal to it, or MARK (more often where the refined
    one is); every other byte random -- only cost_best may matter"""
    out = []
    for a in (pus, pus_small):
        m = np.frombuffer(rng.bytes(a.size * 16), MDT).reshape(a.shape).copy()
        rc = a["cost_best"].astype(np.int64)
        base = np.where(rc == MARK, rng.integers(50, 5000, size=rc.shape), rc)
        c = np.clip(base + rng.choice([-40, -3, -1, 0, 0, 1, 3, 40], size=rc.shape), 0, MARK - 1)
        c = np.where(rng.random(rc.shape) < np.where(rc == MARK, 0.5, 0.25), MARK, c)
        m["cost_best"] = c.astype(np.uint32)
        out.append(m)
    return tuple(out)


def part_combinations(pus, pus_small, merge_pus, merge_small, W, H, rows=None):
    """per level 0..3 the set of (refined available, merge available) pairs seen on parts of INSIDE nodes"""
    cw = (W + 63) // 64
    rb = rows[0] if rows is not None else 0
    seen = {l: set() for l in range(4)}
    fam = {"pu": (pus["cost_best"], merge_pus["cost_best"]), "small": (pus_small["cost_best"], merge_small["cost_best"])}
    for i in range(pus.shape[1]):
        ctu = rb * cw + i
        vw, vh = min(64, W - (ctu % cw) * 64), min(64, H - (ctu // cw) * 64)
        for k in range(85):
            x, y, n = sr.node_rect(k)
            if x + n > vw or y + n > vh:
                continue
            for p in (1, 2, 4, 5, 6, 7):
                w = sr.parts(k, p)
                if w is not None:
                    a, m = fam[w[0]]
                    for e in w[1:]:
                        seen[sr.level(k)] |= set(zip((a[:, i, e] != MARK).tolist(), (m[:, i, e] != MARK).tolist()))
    return seen


# ---- what the constructed pictures of tests/motion_merge_cases.py must show per PU (the CPU test on the restatement, the GPU test on the device) ------

def check_half_sample(got, family, W, H, q, c1):
    """got [numCtus, 124 or 384] of the half-sample picture, every refined node at q: every PU with an available neighbour inherits q at no distortion for
    one bit from the first available position -- every later one holds the same vector and is pruned against L or A, or is the node of L or A itself --;
    a PU with none takes the zero vector alone"""
    ch = (H + 63) // 64
    merged = alone = 0
    for c in range(got.shape[0]):
        for e, (k, s, p) in enumerate(FAMILIES[family][0]()):
            r = got[c, e]
            avail = [j for j, nb in enumerate(candidates(W, H, (0, ch), c, k, s, p)) if nb is not None]
            if avail:
                assert (r["satd_best"], r["cost_best"], r["idx"], r["num"], r["mvx"], r["mvy"], r["src"]) == (0, c1, 0, 2, q[0], q[1], avail[0]), (c, k, s, p, r)
                merged += 1
            else:
                assert (r["src"], r["idx"], r["num"], r["mvx"], r["mvy"]) == (mg.ZERO, 0, 1, 0, 0) and r["satd_best"] > 0, (c, k, s, p, r)
                alone += 1
    assert merged > 0 and alone > 0
    return merged, alone


def check_two_motions(got_pus, refined_pus, v2q, c):
    """got_pus [3, 124] merge records and refined_pus [3, 124] refined PUs of the two-motion pair (CTU 0 moves by V1, CTUs 1 and 2 by V2; v2q: V2 in quarter
    samples, c: the bit costs 0..4), on the PUs of the 64x64 CUs (entries 0..11: shape * 2 + part):
      CTU 2, beyond the boundary: every part whose L sample lies in CTU 1 inherits V2 from its 64x64 node at no distortion for one bit -- cheaper than its
      own vector --; part 1 of the three vertical shapes has its L sample in its own CU and nothing above: the zero vector alone, which does not fit;
      CTU 1, at the boundary: L is CTU 0's node, which moves by V1 -- the parts need V2, and neither V1 nor the zero vector fits: no part merges"""
    for s in range(6):
        for p in range(2):
            e, r2, r1 = 2 * s + p, got_pus[2, 2 * s + p], got_pus[1, 2 * s + p]
            own_l = p == 1 and s in (1, 4, 5)
            if own_l:
                assert (r2["num"], r2["src"]) == (1, mg.ZERO) and r2["cost_best"] > refined_pus["cost_best"][2, e], (s, p, r2)
                assert (r1["num"], r1["src"]) == (1, mg.ZERO), (s, p, r1)
            else:
                assert (r2["src"], r2["idx"], r2["num"], r2["mvx"], r2["mvy"], r2["satd_best"], r2["cost_best"]) == (mg.L, 0, 2, v2q[0], v2q[1], 0, c[1]), (s, p, r2)
                assert r2["cost_best"] < refined_pus["cost_best"][2, e]
                assert r1["num"] == 2
            assert r1["satd_best"] > 0 and r1["cost_best"] > refined_pus["cost_best"][1, e], (s, p, r1)
