"""The constructed pictures of the merge stage's tests, and what the CPU restatements make of them (tests/test_motion_merge_ref.py confirms the expected
values without a GPU; tests/test_gpu_motion_merge.py runs the device on the same pictures).

The half-sample picture: the current picture IS the reference filtered at a half-sample offset and displaced by an integer vector, as
tests/test_motion_refine_ref.py builds it; every node refines to that one vector, so every node with a neighbour inherits it at no distortion.

The two-motion pair: 192 x 64 = three whole CTUs of noise; CTU 0 is the reference displaced by V1, CTUs 1 and 2 the reference displaced by V2, both
integer and non-zero, so every node that lies in one CTU refines to its CTU's vector at SATD 0 and costs the vector's bits alone.  The 64x64 node of CTU 1
has CTU 0's node as its only neighbour (L), which moves differently: it does not merge.  The 64x64 node of CTU 2 inherits V2 from CTU 1 for one bit.
A plain module, not a conftest and not a test."""
import numpy as np

import motion_merge_ref as mg
import motion_range_sweep as sw
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
import p_tree_ref as tr
import pu_shape_ref as sr
from pu_shape_cases import displaced

W, H, QP, RANGE = 192, 64, 30, 4
V1, V2 = (2, 1), (-3, 2)
HALF_CASES = [(8, 2, 0, (3, -2)), (10, 2, 2, (0, 0)), (12, 0, 2, (-5, 1))]      # bit depth, fraction (fx, fy), integer vector
HALF_W, HALF_H, HALF_QP = 192, 128, 4
_CACHE = {}


def half_sample_case(bd, fx, fy, mv):
    """-> dict(ref, cur [H, W] int64, planes, q: the true vector in quarter samples, refined [numCtus, 85] MOTION_QPEL_DTYPE: every node at q)"""
    key = ("half", bd, fx, fy, mv)
    if key not in _CACHE:
        rng = np.random.default_rng(21 + bd)
        yy, xx = np.mgrid[0:HALF_H, 0:HALF_W]
        v = (0.5 + 0.3 * np.sin(xx / 11.0) * np.cos(yy / 7.0)) * ((1 << bd) - 1) + rng.normal(0, 40 << (bd - 8), size=(HALF_H, HALF_W))
        ref = np.clip(np.rint(v), 0, (1 << bd) - 1).astype(np.int64)
        planes = mr.Planes(ref, bd, 16)
        tx, ty = 4 * mv[0] + fx, 4 * mv[1] + fy
        y, x = planes.pad + (ty >> 2), planes.pad + (tx >> 2)
        cur = planes.planes[ty & 3][tx & 3][y:y + HALF_H, x:x + HALF_W].astype(np.int64)
        refined = np.zeros((6, 85), mg.capi.MOTION_QPEL_DTYPE)
        refined["mvx"], refined["mvy"], refined["cost_best"] = tx, ty, 1234
        _CACHE[key] = dict(ref=ref, cur=cur, planes=planes, q=(tx, ty), refined=refined)
    return _CACHE[key]


def check_half_sample(got, q, c1):
    """got [6, 85] merge records of the 3 x 2 CTU picture: every node with an available neighbour inherits q at no distortion for one bit, from L -- or,
    in the picture's first column, from A; the first node of every level has no neighbour and takes the zero vector"""
    checked = 0
    for c in range(6):
        for k in range(85):
            lvl, bx, by = mr.node_geometry(k)
            gx, gy = (c % 3) * (1 << lvl) + bx, (c // 3) * (1 << lvl) + by
            r = got[c, k]
            if gx == 0 and gy == 0:
                assert (r["src"], r["idx"], r["num"], r["mvx"], r["mvy"]) == (mg.ZERO, 0, 1, 0, 0) and r["satd_best"] > 0, (c, k, r)
            else:
                # the neighbours all carry q: A, AR, BL and AL are pruned against L (or AR and AL against A), the zero vector closes the list
                assert (r["satd_best"], r["cost_best"], r["idx"], r["num"], r["mvx"], r["mvy"]) == (0, c1, 0, 2, q[0], q[1]), (c, k, r)
                assert r["src"] == (mg.A if gx == 0 else mg.L), (c, k, r)
            checked += 1
    assert checked == 6 * 85


def pictures():
    """(cur, ref) uint8 [H, W] of the two-motion pair"""
    if "pics" not in _CACHE:
        rng = np.random.default_rng(1905)
        ref = rng.integers(0, 256, size=(H, W)).astype(np.int64)
        cur = displaced(ref, *V2)
        cur[:, :64] = displaced(ref, *V1)[:, :64]
        _CACHE["pics"] = (cur.astype(np.uint8), ref.astype(np.uint8))
    return _CACHE["pics"]


def two_motion_case(oracle):
    """the pair through the CPU restatements: SAD searches at range 4 (motion_range_sweep), quarter-sample refinements (motion_refine_ref,
    motion_refine_pu_ref), the selection (pu_shape_ref), the merge stage (motion_merge_ref) and both trees, default rules -> dict(refined, shapes, merge
    [3, 85], plain / merged: (records [3, 85], dmin, dmax [3, 256]), vector_cost(ctu, mvx, mvy) of an integer vector (the same for every CTU here), c: bit costs 0..4)"""
    if "case" not in _CACHE:
        cur, ref = (p.astype(np.int64) for p in pictures())
        found = sw.PairSweep(oracle, cur, ref, 8, QP, sad=True, rmax=RANGE).records(RANGE)
        cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
        planes = mr.Planes(ref, 8, RANGE + 8)
        refined = {"nodes": mr.expected(oracle, cur_flat, 0, W, ref, W, H, 8, QP, found["nodes"], RANGE, planes=planes),
                   "pu": rp.expected(oracle, cur, ref, 8, QP, found["pu"], RANGE, "pu", planes=planes),
                   "small": rp.expected(oracle, cur, ref, 8, QP, found["small"], RANGE, "small", planes=planes)}
        shapes, _ = sr.select(refined["nodes"][None], refined["pu"][None], refined["small"][None], W, H)
        merge = mg.expected(oracle, cur_flat, 0, W, ref, W, H, 8, QP, refined["nodes"], RANGE, planes=planes)
        sl = mr.sqrt_lambda(oracle, QP, 8)
        _CACHE["case"] = dict(refined=refined, found=found, shapes=shapes[0], merge=merge, plain=tuple(a[0] for a in tr.select(shapes, W, H)),
                              merged=tuple(a[0] for a in mg.tree_select(shapes, merge[None], W, H)),
                              vector_cost=lambda ctu, mvx, mvy: mr.qpel_cost(4 * mvx, 4 * mvy, sl), c=[mg.bit_cost(b, sl) for b in range(5)])
    return _CACHE["case"]


COARSE, CENTRED_RANGE, CENTRED_MERGE_RANGE = 1, 8, 64      # the centred chain: centres within +-4 samples, so +-8 around any of them holds V1 and V2


def two_motion_centred_case(oracle):
    """the same pair through the restatements of the centred chain (motion_centred_ref: one coarse centre per CTU at coarse range 1, the searches and
    refinements at range 8 around it), the selection, the merge stage at max_range 64 -- absolute vectors, neighbouring CTUs with different centres -- and both
    trees -> two_motion_case's dict, with centres [3] and vector_cost(ctu, mvx, mvy): of an integer vector priced against that CTU's centre"""
    if "centred" not in _CACHE:
        import motion_centred_ref as cr
        cur, ref = (p.astype(np.int64) for p in pictures())
        centres = cr.centres(cur, ref, 8, cr.sqrt_lambda(QP), COARSE)
        found = cr.centred_search(oracle, cur, ref, 8, QP, CENTRED_RANGE, centres)
        refined = cr.centred_refine(oracle, cur, ref, 8, QP, CENTRED_RANGE, centres, found)
        shapes, _ = sr.select(refined["nodes"][None], refined["pu"][None], refined["small"][None], W, H)
        cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
        merge = mg.expected(oracle, cur_flat, 0, W, ref, W, H, 8, QP, refined["nodes"], CENTRED_MERGE_RANGE)
        sl = mr.sqrt_lambda(oracle, QP, 8)
        P = [(int(centres["mvx"][c]), int(centres["mvy"][c])) for c in range(3)]
        _CACHE["centred"] = dict(centres=centres, refined=refined, found=found, shapes=shapes[0], merge=merge, plain=tuple(a[0] for a in tr.select(shapes, W, H)),
                                 merged=tuple(a[0] for a in mg.tree_select(shapes, merge[None], W, H)),
                                 vector_cost=lambda ctu, mvx, mvy: mr.qpel_cost(4 * (mvx - P[ctu][0]), 4 * (mvy - P[ctu][1]), sl),
                                 c=[mg.bit_cost(b, sl) for b in range(5)])
    return _CACHE["centred"]


def check_two_motions(refined_nodes, merge, tree, dmin, dmax, vector_cost, c):
    """what the pair must show, on records [3, 85] and maps [3, 256] of a chain WITH the merge stage; vector_cost(ctu, mvx, mvy): what the chain's refinement
    charges a CTU's nodes for an integer vector (the zero-centred chain: against zero; the centred chain: against the CTU's centre)"""
    v1, v2a, v2b = vector_cost(0, *V1), vector_cost(1, *V2), vector_cost(2, *V2)
    # every 64x64 node found its CTU's motion with nothing left
    for ctu, v, cost in ((0, V1, v1), (1, V2, v2a), (2, V2, v2b)):
        r = refined_nodes[ctu, 0]
        assert (r["mvx"], r["mvy"], r["satd_best"], r["cost_best"]) == (4 * v[0], 4 * v[1], 0, cost), (ctu, r)
    # CTU 1: its only neighbour moves differently -> L (V1) and the zero vector, both far from the content; the explicit vector stays
    m1, m2 = merge[1, 0], merge[2, 0]
    assert m1["num"] == 2 and m1["cost_best"] > v2a and m1["satd_best"] > 0
    assert not tree["flags"][1, 0] & mg.MERGED and tree["cost_own"][1, 0] == v2a
    # CTU 2 inherits V2 from CTU 1 for one bit: its refined cost minus the vector's bits plus c[1]
    assert (m2["src"], m2["idx"], m2["num"], m2["mvx"], m2["mvy"], m2["satd_best"]) == (mg.L, 0, 2, 4 * V2[0], 4 * V2[1], 0), m2
    assert m2["cost_best"] == int(refined_nodes["cost_best"][2, 0]) - v2b + c[1] == c[1]
    assert tree["flags"][2, 0] & mg.MERGED and tree["cost_own"][2, 0] == c[1] and c[1] < v2b
    # CTU 0 has no neighbour at all at its first node: the zero vector alone, which loses to the explicit vector
    assert merge["num"][0, 0] == 1 and merge["src"][0, 0] == mg.ZERO and not tree["flags"][0, 0] & mg.MERGED
    # the expected map: no CTU is split -- a uniformly moving CTU costs one vector (or one merge bit) as a whole and at least two as quarters
    assert not dmin.any() and not dmax.any()
    assert (tree["cost_tree"][:, 0] == tree["cost_own"][:, 0]).all()
    # hand-computed: the children of CTU 1's root -- (0, 0) keeps its vector (L moves with V1), (1, 0) and (1, 1) inherit from L for one bit, (0, 1) from A
    # (list position 1: L is CTU 0's V1) for two
    assert [int(v) for v in tree["cost_own"][1, 1:5]] == [v2a, c[1], c[2], c[1]]
    assert int(tree["cost_kids"][1, 0]) == v2a + 2 * c[1] + c[2]
