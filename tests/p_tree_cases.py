"""The picture pair of the tree decision's pipeline test, and what the CPU restatements make of it (tests/test_p_tree_ref.py confirms the expected map
without a GPU; tests/test_gpu_p_tree.py runs the device chains on the same pair).

A 104 x 88 pair of noise texture (a 2 x 2 CTU grid with one whole CTU): the current picture is the reference displaced by (2, 1) with a little noise on
top, except for CTU 0, which is built from integer displacements of the reference alone, so that every block that covers one motion refines to SATD 0 at
that vector and costs its vector alone:
  the whole CTU moves by (2, 1);
  the four 16x16 blocks of the 32x32 CU at (32, 32) move, in raster order, by (3, 0), (-2, 1), (1, -3), (-4, -2);
  the four 8x8 blocks of the 16x16 CU at (0, 0) move by (5, 2), (0, 3), (-3, 0), (1, 1).
The cheapest tree of CTU 0 is therefore: 32x32 CUs at (32, 0) and (0, 32), 16x16 CUs in the quadrants at (32, 32) and (0, 0), and 8x8 CUs in the 16x16 at
(0, 0); its cost is the sum of the vector costs of its 15 CUs.  A plain module, not a conftest and not a test."""
import numpy as np

import motion_range_sweep as sw
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
import p_tree_ref as tr
import pu_shape_ref as sr
from pu_shape_cases import displaced

W, H, QP, RANGE = 104, 88, 30, 8
COARSE = 4                                           # the coarse range of the centred chain
PAN = (2, 1)
MOVES_16 = ((3, 0), (-2, 1), (1, -3), (-4, -2))      # the 16x16 blocks of the 32x32 CU at (32, 32), raster order
MOVES_8 = ((5, 2), (0, 3), (-3, 0), (1, 1))          # the 8x8 blocks of the 16x16 CU at (0, 0), raster order
_CACHE = {}


def pictures():
    """(cur, ref) uint8 [H, W]"""
    if "pics" not in _CACHE:
        rng = np.random.default_rng(77)
        ref = rng.integers(0, 256, size=(H, W)).astype(np.int64)
        cur = np.clip(displaced(ref, *PAN) + rng.integers(-2, 3, size=(H, W)), 0, 255)
        yy, xx = np.mgrid[0:H, 0:W]

        def move(region, mv):
            cur[region] = displaced(ref, *mv)[region]

        move((xx < 64) & (yy < 64), PAN)
        for i, mv in enumerate(MOVES_16):
            x, y = 32 + 16 * (i & 1), 32 + 16 * (i >> 1)
            move((xx >= x) & (xx < x + 16) & (yy >= y) & (yy < y + 16), mv)
        for i, mv in enumerate(MOVES_8):
            x, y = 8 * (i & 1), 8 * (i >> 1)
            move((xx >= x) & (xx < x + 8) & (yy >= y) & (yy < y + 8), mv)
        _CACHE["pics"] = (cur.astype(np.uint8), ref.astype(np.uint8))
    return _CACHE["pics"]


def expected_map_ctu0():
    """depth_min == depth_max of CTU 0, [16, 16]"""
    m = np.zeros((16, 16), np.uint8)
    m[0:8, 8:16] = 1          # the quadrant at (32, 0)
    m[8:16, 0:8] = 1          # ... at (0, 32)
    m[8:16, 8:16] = 2         # ... at (32, 32): four 16x16 CUs
    m[0:8, 0:8] = 2           # ... at (0, 0): 16x16 CUs,
    m[0:4, 0:4] = 3           # except the 16x16 at (0, 0): four 8x8 CUs
    return m.reshape(256)


def expected_tree_cost(vector_cost):
    """cost_tree of CTU 0's root: five CUs that move with the pan (two 32x32, three 16x16), the four 16x16 and the four 8x8 with their own vectors"""
    return 5 * vector_cost(*PAN) + sum(vector_cost(*v) for v in MOVES_16) + sum(vector_cost(*v) for v in MOVES_8)


def constructed_case(oracle):
    """the 8-bit pair through the CPU restatements: SAD searches at range 8 (motion_range_sweep), quarter-sample refinements (motion_refine_ref,
    motion_refine_pu_ref), the selection (pu_shape_ref) and the tree (p_tree_ref), default rules -> dict(shapes [numCtus, 85], tree [numCtus, 85],
    dmin / dmax [numCtus, 256], refined, vector_cost(mvx, mvy): of an integer vector)"""
    if "case" not in _CACHE:
        cur, ref = (p.astype(np.int64) for p in pictures())
        found = sw.PairSweep(oracle, cur, ref, 8, QP, sad=True, rmax=RANGE).records(RANGE)
        cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
        planes = mr.Planes(ref, 8, RANGE + 8)
        refined = {"nodes": mr.expected(oracle, cur_flat, 0, W, ref, W, H, 8, QP, found["nodes"], RANGE, planes=planes),
                   "pu": rp.expected(oracle, cur, ref, 8, QP, found["pu"], RANGE, "pu", planes=planes),
                   "small": rp.expected(oracle, cur, ref, 8, QP, found["small"], RANGE, "small", planes=planes)}
        shapes, _ = sr.select(refined["nodes"][None], refined["pu"][None], refined["small"][None], W, H)
        tree, dmin, dmax = tr.select(shapes, W, H)
        sl = mr.sqrt_lambda(oracle, QP, 8)
        _CACHE["case"] = dict(shapes=shapes[0], tree=tree[0], dmin=dmin[0], dmax=dmax[0], refined=refined, found=found,
                              vector_cost=lambda mvx, mvy: mr.qpel_cost(4 * mvx, 4 * mvy, sl))
    return _CACHE["case"]


def centred_case(oracle):
    """the same pair through the restatements of the centred chain (motion_centred_ref: one coarse centre per CTU at coarse range 4, the searches and
    refinements around it), the selection and the tree -> dict(centres [numCtus], shapes, tree, dmin, dmax, refined, vector_cost(mvx, mvy): of an
    integer vector of CTU 0, which is priced relative to that CTU's centre)"""
    if "centred" not in _CACHE:
        import motion_centred_ref as cr
        cur, ref = (p.astype(np.int64) for p in pictures())
        centres = cr.centres(cur, ref, 8, cr.sqrt_lambda(QP), COARSE)
        found = cr.centred_search(oracle, cur, ref, 8, QP, RANGE, centres)
        refined = cr.centred_refine(oracle, cur, ref, 8, QP, RANGE, centres, found)
        shapes, _ = sr.select(refined["nodes"][None], refined["pu"][None], refined["small"][None], W, H)
        tree, dmin, dmax = tr.select(shapes, W, H)
        sl = mr.sqrt_lambda(oracle, QP, 8)
        px, py = int(centres["mvx"][0]), int(centres["mvy"][0])
        _CACHE["centred"] = dict(centres=centres, shapes=shapes[0], tree=tree[0], dmin=dmin[0], dmax=dmax[0], refined=refined, found=found,
                                 vector_cost=lambda mvx, mvy: mr.qpel_cost(4 * (mvx - px), 4 * (mvy - py), sl))
    return _CACHE["centred"]


def check_constructed(tree, dmin, dmax, vector_cost):
    """what the constructed pair must show with the default rules, on records [numCtus, 85] and maps [numCtus, 256]"""
    assert np.array_equal(dmin, dmax), "the default rule is the hard decision"
    exp = expected_map_ctu0()
    assert np.array_equal(dmin[0], exp), (dmin[0].reshape(16, 16), exp.reshape(16, 16))
    assert int(tree["cost_tree"][0, 0]) == expected_tree_cost(vector_cost), (int(tree["cost_tree"][0, 0]), expected_tree_cost(vector_cost))
    assert int(tree["cost_own"][0, 0]) > int(tree["cost_tree"][0, 0])
    # the ragged CTUs (40 wide, 24 tall) are split at the edge and hold zeros outside the picture
    for c in (1, 2, 3):
        vw, vh = tr.valid_size(c, W, H)
        m = dmin[c].reshape(16, 16)
        assert (m[:, vw // 4:] == 0).all() and (m[vh // 4:, :] == 0).all() and (m[:vh // 4, :vw // 4] >= 1).all(), (c, m)
        assert tree["flags"][c, 0] & tr.CROSSING
