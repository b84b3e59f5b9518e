"""The constructed inputs of the max_range sweep through the merge stages and the zero-residual stage (k_motion_merge.hip, k_motion_merge_pu.hip,
k_motion_skip.hip: the three users of refine_stage_window_reach), and what the CPU restatements make of them.  tests/test_motion_merge_range_sweep_ref.py
asserts without a GPU that these inputs probe what they are meant to probe; tests/test_gpu_motion_merge_range_sweep.py runs the device on them.

The picture is 168 x 152 = 3 x 3 CTUs: four whole 64x64 nodes, of which three have a left, an above or a diagonal neighbour, a column 40 samples
wide, a row 24 samples tall and the corner; at every range the windows reach the replicated border on some side.

Corner pairs: the reference is noise, the current picture the reference's own prediction at q = (sx (4R + 3), sy (4R + 3)), the four corners of the
reach of max_range R, and every refined record carries q: every node or PU with an available neighbour inherits q at distortion 0 for one bit, and any
sample that differs from the restatement's makes its distortion non-zero.  -(4R + 3) reads the first row and column of the staged part of the window for
their value and +(4R + 3) the last (staged_part and read_for_value below; -+(4R + 2) read them too, +-(4R + 1) and +-4R do not: their outer tap is 0).

The draw: noise pictures and refined records from motion_merge_pu_ref.random_refined with a pool that holds all four corners of the reach, its edges
and the vectors just inside it; skip inputs are the expected merge records, and a second set in test_gpu_motion_skip.random_merge's scheme.

Content: a workgroup that staged the same reference at a larger range before leaves the right samples behind in the LDS cells a later, smaller range
does not stage, so no two launches may show the same reference samples: every picture is seeded by (kind, variant, bit depth, R).
A plain module, not a conftest and not a test."""
import numpy as np

import motion_merge_pu_ref as mpu
import motion_merge_ref as mg
import motion_pu_ref as mp
import motion_refine_ref as mr
import motion_skip_ref as sk

W, H = 168, 152
CW, CH = 3, 3
N = CW * CH
PAD = 72                                        # >= 64 + 6: one Planes object serves every range
RANGES = tuple(range(1, 65))
BIT_DEPTHS = (8, 10, 12)
CORNERS = ((1, 1), (-1, 1), (1, -1), (-1, -1))
CORNER_QP = {8: 30, 10: 34, 12: 26}             # the one-bit cost is well above zero: a winner's cost_best is not its satd_best
DRAW_QP, SKIP_QP = 4, 30                        # bits are cheap at qp 4: any list position can win
KINDS = {"corner": 1, "draw": 2, "unrelated": 3}
VARIANTS = {"sweep": 0, "guarded": 1, "changing": 2, "host": 3}
MDT, QDT, KDT = mg.MDT, mpu.QDT, sk.SDT
_CACHE = {}


def seed(kind, variant, bd, R, extra=0):
    return [20261, KINDS[kind], VARIANTS[variant], bd, R, extra]


def noise(kind, variant, bd, R, extra=0):
    return np.random.default_rng(seed(kind, variant, bd, R, extra)).integers(0, 1 << bd, size=(H, W)).astype(np.int64)


# ---- geometry: which entries have an available neighbour, from the picture alone --------------------------------------------------------------------

def level_of(family, e):
    k = e if family == "nodes" else mpu.FAMILIES[family][0]()[e][0]
    return mr.node_geometry(k)[0]


def rect_in_ctu(family, e):
    """(x0, y0, w, h) of an entry inside its CTU"""
    if family == "nodes":
        lvl, bx, by = mr.node_geometry(e)
        n = 64 >> lvl
        return bx * n, by * n, n, n
    return mp.pu_rect(*mpu.FAMILIES[family][0]()[e])


def geometry():
    """-> {family: (valid [N, entries] bool: the entry's CU node is INSIDE, fed [N, entries] bool: valid and at least one candidate position holds an
    addressable neighbour)} for "nodes", "pu" and "small", whole picture"""
    if "geometry" not in _CACHE:
        out = {}
        valid, fed = np.zeros((N, 85), bool), np.zeros((N, 85), bool)
        for c in range(N):
            for k in range(85):
                lvl, bx, by = mr.node_geometry(k)
                gx, gy = (c % CW) * (1 << lvl) + bx, (c // CW) * (1 << lvl) + by
                valid[c, k] = mg.inside(W, H, lvl, gx, gy)
                fed[c, k] = valid[c, k] and any(nb is not None for nb in mg.neighbours(W, H, (0, CH), lvl, gx, gy))
        out["nodes"] = (valid, fed)
        for fam, (cov, n) in mpu.FAMILIES.items():
            v, f = np.zeros((N, n), bool), np.zeros((N, n), bool)
            for c in range(N):
                for e, (k, s, p) in enumerate(cov()):
                    lvl, (gx, gy), _ = mpu.pu_geometry(W, c, k, s, p)
                    v[c, e] = mg.inside(W, H, lvl, gx, gy)
                    f[c, e] = v[c, e] and any(nb is not None for nb in mpu.candidates(W, H, (0, CH), c, k, s, p))
            out[fam] = (v, f)
        _CACHE["geometry"] = out
    return _CACHE["geometry"]


def level_counts():
    """-> {(family, level): (fed, valid)}: how many entries of a level inherit, of how many valid ones"""
    out = {}
    for fam, (valid, fed) in geometry().items():
        lv = np.array([level_of(fam, e) for e in range(valid.shape[1])])
        for l in sorted(set(lv.tolist())):
            out[(fam, l)] = (int(fed[:, lv == l].sum()), int(valid[:, lv == l].sum()))
    return out


def on_the_side(family, e, sx, sy):
    """the entry's rectangle touches the sides of its CTU that (sx, sy) point to: its prediction reads that end of the window"""
    x0, y0, w, h = rect_in_ctu(family, e)
    return (x0 + w == 64 if sx > 0 else x0 == 0) and (y0 + h == 64 if sy > 0 else y0 == 0)


# ---- corner pairs -----------------------------------------------------------------------------------------------------------------------------------

def corner_vector(R, corner):
    return corner[0] * (4 * R + 3), corner[1] * (4 * R + 3)


def corner_pictures(bd, R, variant="sweep", extra=0):
    """-> (ref [H, W] int64 noise, planes): one Planes object per reference picture, for all four corners and all three restatements"""
    ref = noise("corner", variant, bd, R, extra)
    return ref, mr.Planes(ref, bd, PAD)


def predicted(planes, q):
    """the picture that is the reference's own prediction at q"""
    y, x = planes.pad + (q[1] >> 2), planes.pad + (q[0] >> 2)
    return planes.planes[q[1] & 3][q[0] & 3][y:y + H, x:x + W].astype(np.int64)


def corner_refined(q):
    refined = np.zeros((N, 85), QDT)
    refined["mvx"], refined["mvy"], refined["cost_best"] = q[0], q[1], 1234
    return refined


def flat16(pic):
    return np.ascontiguousarray(np.asarray(pic).astype(np.int16)).reshape(-1)


def expected_all(oracle, cur, ref, planes, bd, merge_qp, skip_qp, refined, R):
    """the three restatements on one pair -> dict(nodes, pu, small: merge records; skip: the skip records at the vectors of `nodes`)"""
    cf = flat16(cur)
    out = {"nodes": mg.expected(oracle, cf, 0, W, ref, W, H, bd, merge_qp, refined, R, planes=planes)}
    for fam in ("pu", "small"):
        out[fam] = mpu.expected(oracle, cf, 0, W, ref, W, H, bd, merge_qp, refined, R, fam, planes=planes)
    out["skip"] = sk.expected(cur, ref, W, H, bd, skip_qp, out["nodes"], R, planes=planes)
    return out


def corner_case(oracle, bd, R, variant="sweep", extra=0, corners=CORNERS):
    """-> dict(ref, qp, c1: the one-bit cost, corners: {corner: dict(q, cur, refined, exp: expected_all's dict)}); the sweep's own cases (all four corners,
    extra 0) are kept, without their pictures; extra: another picture for the same (variant, bit depth, R)"""
    key = ("corner", bd, R, variant)
    if key in _CACHE and extra == 0:
        kept = _CACHE[key]
        ref, planes = corner_pictures(bd, R, variant)
        return dict(kept, ref=ref, corners={c: dict(v, cur=predicted(planes, v["q"])) for c, v in kept["corners"].items() if c in corners})
    ref, planes = corner_pictures(bd, R, variant, extra)
    qp = CORNER_QP[bd]
    wanted, corners = corners, {}
    for corner in wanted:
        q = corner_vector(R, corner)
        cur, refined = predicted(planes, q), corner_refined(q)
        corners[corner] = dict(q=q, cur=cur, refined=refined, exp=expected_all(oracle, cur, ref, planes, bd, qp, SKIP_QP, refined, R))
    case = dict(ref=ref, qp=qp, c1=mg.bit_cost(1, mr.sqrt_lambda(oracle, qp, bd)), corners=corners)
    if variant == "sweep" and extra == 0 and tuple(wanted) == CORNERS:
        _CACHE[key] = dict(qp=qp, c1=case["c1"], corners={c: {k: v[k] for k in ("q", "refined", "exp")} for c, v in corners.items()})
    return case


def check_corner(got, q, c1):
    """got: dict(nodes, pu, small, skip) of records [N, entries] of a corner pair, from a restatement or from the device, against the closed form: every
    fed entry inherits q at distortion 0 for one bit as the first of two list entries, every other valid entry takes the zero vector alone; the skip
    stage finds no coefficient where the node inherited -> {family: fed entries checked}"""
    n = {}
    for fam, (valid, fed) in geometry().items():
        r = got[fam]
        assert r.shape == valid.shape, (fam, r.shape)
        for f, want in (("satd_best", 0), ("cost_best", c1), ("mvx", q[0]), ("mvy", q[1]), ("idx", 0), ("num", 2)):
            bad = fed & (r[f] != want)
            assert not bad.any(), (fam, q, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), r[f][bad][:5].tolist())
        alone = valid & ~fed
        assert (r["src"][fed] != mg.ZERO).all() and (r["src"][alone] == mg.ZERO).all() and (r["num"][alone] == 1).all(), (fam, q)
        assert (r["mvx"][alone] == 0).all() and (r["mvy"][alone] == 0).all() and (r["satd_best"][alone] > 0).all(), (fam, q)
        assert (r["cost_best"][~valid] == mg.MARK).all() and (r["num"][~valid] == 0).all(), (fam, q)
        n[fam] = int(fed.sum())
    valid, fed = geometry()["nodes"]
    s = got["skip"]
    bad = fed & ((s["coef_max"] != 0) | (s["flags"] != 3) | (s["level_sum"] != 0) | (s["nonzero"] != 0) | (s["mvx"] != q[0]) | (s["mvy"] != q[1]))
    assert not bad.any(), ("skip", q, int(bad.sum()), np.argwhere(bad)[:5].tolist(), s["coef_max"][bad][:5].tolist())
    assert (s["coef_max"][valid & ~fed] > 0).all() and (s["coef_max"][~valid] == sk.MARK).all(), ("skip", q)
    n["skip"] = int(fed.sum())
    return n


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------------------

def draw_pool(R):
    """the vectors the draw's refined records come from: motion_merge_pu_ref.random_refined's near ones (three times each, so that equal neighbours stay
    frequent), all four corners of the reach, its four edges at a small other component, and the magnitudes just inside it"""
    reach = 4 * R + 3
    near = [(-5, 2), (3, 3), (0, -7)]
    corners = [(reach, -reach), (reach, reach), (-reach, reach), (-reach, -reach)]
    edges = [(reach, 2), (-reach, -1), (1, reach), (-3, -reach)]
    inner = [(reach - 1, -(reach - 2)), (-(reach - 1), reach - 2), (reach - 2, reach - 1), (-(reach - 2), -(reach - 1)), (4 * R, -4 * R), (-4 * R, 4 * R)]
    return near * 3 + corners + edges + inner


def random_merge(rng, shape, max_range):
    """test_gpu_motion_skip.random_merge's scheme: vectors anywhere within the reach, one in ten on its limit, one in ten beyond it (by one quarter sample,
    or anywhere), one in seven marked"""
    from test_gpu_motion_skip import random_merge as scheme
    return scheme(rng, shape, max_range)


def draw_refined(R):
    return mpu.random_refined(np.random.default_rng([77, R]), (N, 85), R, pool=draw_pool(R))


def draw_case(oracle, bd, R, variant="sweep"):
    """-> dict(pics: (ref, cur) noise, refined [N, 85], exp: expected_all's dict at DRAW_QP / SKIP_QP, merge2 [N, 85]: merge records in random_merge's
    scheme, skip2: the skip records at them); the refined and merge2 records depend on R alone"""
    key = ("draw", bd, R, variant)
    if key in _CACHE:
        kept = _CACHE[key]
        return dict(kept, pics=(noise("draw", variant, bd, R, 0), noise("draw", variant, bd, R, 1)))
    ref, cur = noise("draw", variant, bd, R, 0), noise("draw", variant, bd, R, 1)
    planes = mr.Planes(ref, bd, PAD)
    refined = draw_refined(R)
    exp = expected_all(oracle, cur, ref, planes, bd, DRAW_QP, SKIP_QP, refined, R)
    merge2 = random_merge(np.random.default_rng([78, R]), (N, 85), R)
    skip2 = sk.expected(cur, ref, W, H, bd, SKIP_QP, merge2, R, planes=planes)
    case = dict(pics=(ref, cur), refined=refined, exp=exp, merge2=merge2, skip2=skip2)
    if variant == "sweep":
        _CACHE[key] = {k: case[k] for k in ("refined", "exp", "merge2", "skip2")}
    return case


# ---- the index arithmetic of refine_stage_window_reach, and the cells refine_tile_diff reads for their value --------------------------------------------

def staged_part(MR, R):
    """-> (rows, columns) of the LDS window of layout MR that refine_stage_window_reach writes at max_range R, as sorted integer arrays"""
    RP = 64 + 2 * MR + 8
    skip = MR - R
    c0 = skip >> 2
    rows, ch = RP - 2 * skip, RP // 4 - 2 * c0
    it = np.arange(rows * ch)
    r = it // ch
    return np.unique(skip + r), np.unique(((c0 + it - r * ch) * 4)[:, None] + np.arange(4)[None, :])


def read_for_value(MR, q, taps):
    """the window coordinates of one axis whose value enters a prediction at the vector component q (quarter samples): the first tap of sample 0 of the
    tile at position t = 0, 8, .., 56 lies at t + MR + 4 + (q >> 2) - 3, sample x of the tile reads taps j = 0..7 at + x + j, and a tap counts where its
    coefficient is not zero; taps: {fraction: the eight coefficients}"""
    first = np.arange(0, 64, 8)[:, None, None] + MR + 4 + (q >> 2) - 3
    used = np.array([j for j in range(8) if taps[q & 3][j] != 0])
    return np.unique(first + np.arange(8)[None, :, None] + used[None, None, :])


def draw_statistics(refined, R, family):
    """-> (set of list lengths, {pruning pair: [fired, did not fire]}) of the lists that refined [N, 85] gives a family, as
    motion_merge_pu_ref.list_statistics counts them"""
    if family != "nodes":
        return mpu.list_statistics(W, H, (0, CH), refined, R, family)
    reach = 4 * R + 3
    lengths, pairs = set(), {n: [0, 0] for n in ("A_L", "AR_A", "BL_L", "AL_L", "AL_A")}
    valid, _ = geometry()["nodes"]
    for c in range(N):
        for k in range(85):
            if not valid[c, k]:
                continue
            lvl, bx, by = mr.node_geometry(k)
            v, cands = [], []
            for nb in mg.neighbours(W, H, (0, CH), lvl, (c % CW) * (1 << lvl) + bx, (c // CW) * (1 << lvl) + by):
                r = None if nb is None else refined[nb[0], nb[1]]
                cands.append(None if r is None else (int(r["cost_best"]), int(r["mvx"]), int(r["mvy"])))
                ok = r is not None and r["cost_best"] != mg.MARK and abs(int(r["mvx"])) <= reach and abs(int(r["mvy"])) <= reach
                v.append((int(r["mvx"]), int(r["mvy"])) if ok else None)
            lengths.add(len(mg.build_list(cands, R)))
            for name, a, b in (("A_L", 1, 0), ("AR_A", 2, 1), ("BL_L", 3, 0), ("AL_L", 4, 0), ("AL_A", 4, 1)):
                if v[a] is not None and v[b] is not None:
                    pairs[name][0 if v[a] == v[b] else 1] += 1
    return lengths, pairs
