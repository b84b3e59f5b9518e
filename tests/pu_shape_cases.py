"""The picture pair of the partition-size selection's pipeline test, and what the CPU restatements make of it (tests/test_pu_shape_ref.py confirms
the three constructed CUs without a GPU; tests/test_gpu_pu_shape.py runs the device pipeline on the same pair).

A 104 x 88 pair of noise texture (the size tests/motion_range_sweep.py uses: a 2 x 2 CTU grid with one whole CTU): the current picture is the
reference displaced by (2, 1) with a little noise on top, except for three CUs of the whole CTU that are built from integer displacements of the
reference, so that a PU that covers one motion alone refines to SATD 0 at that vector and costs its vector alone:
  CU_2NxN     the 32x32 CU at (32, 32): top half moves by (+3, 0), bottom half by (-2, +1)
  CU_nLx2N    the 32x32 CU at (0, 0): the left quarter (8 columns) moves by (+1, +2), the rest by (+4, 0)
  CU_Nx2N_16  the 16x16 CU at (32, 0): below its top four rows the left half moves by (+2, +3) and the right half by (0, +1); the top four rows move by
              (+5, +2) as a whole, so 2NxnU (one part exact, the other half right) is cheaper than 2Nx2N (never more than three eighths right)
A plain module, not a conftest and not a test."""
import numpy as np

import motion_range_sweep as sw
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
import pu_shape_ref as sr
from fasthevc_amd import capi

W, H, QP, RANGE = 104, 88, 30, 8
# (CTU, node)
CU_2NxN = (0, 4)
CU_nLx2N = (0, 1)
CU_Nx2N_16 = (0, 7)
# a margin that reaches every available size: what is left of the AMP bits is the gate's doing
WIDE_MARGIN = 0x7FFFFFFF
_CACHE = {}


def displaced(ref, mvx, mvy):
    """ref seen through the integer vector (mvx, mvy), coordinates clamped to the picture (the searches' border replication)"""
    yy, xx = np.mgrid[0:ref.shape[0], 0:ref.shape[1]]
    return ref[np.clip(yy + mvy, 0, ref.shape[0] - 1), np.clip(xx + mvx, 0, ref.shape[1] - 1)]


def pictures():
    """(cur, ref) uint8 [H, W]"""
    if "pics" not in _CACHE:
        rng = np.random.default_rng(2026)
        ref = rng.integers(0, 256, size=(H, W)).astype(np.int64)
        cur = np.clip(displaced(ref, 2, 1) + rng.integers(-2, 3, size=(H, W)), 0, 255)
        yy, xx = np.mgrid[0:H, 0:W]

        def move(region, mv):
            cur[region] = displaced(ref, *mv)[region]

        cu = (xx >= 32) & (xx < 64) & (yy >= 32) & (yy < 64)
        move(cu & (yy < 48), (3, 0))
        move(cu & (yy >= 48), (-2, 1))
        cu = (xx < 32) & (yy < 32)
        move(cu & (xx < 8), (1, 2))
        move(cu & (xx >= 8), (4, 0))
        cu = (xx >= 32) & (xx < 48) & (yy < 16)
        move(cu & (yy < 4), (5, 2))
        move(cu & (yy >= 4) & (xx < 40), (2, 3))
        move(cu & (yy >= 4) & (xx >= 40), (0, 1))
        _CACHE["pics"] = (cur.astype(np.uint8), ref.astype(np.uint8))
    return _CACHE["pics"]


def rules():
    """(the default rule, the wide margin behind the AMP gate, the wide margin without the gate)"""
    return capi.pu_shape_rule_default(), capi.pu_shape_rule(0, WIDE_MARGIN, 1), capi.pu_shape_rule(0, WIDE_MARGIN, 0)


def constructed_case(oracle):
    """the 8-bit pair through the CPU restatements: SAD searches at range 8 (motion_range_sweep), quarter-sample refinements (motion_refine_ref,
    motion_refine_pu_ref), the selection (pu_shape_ref) -> dict(rec, costs: default rule; rec_amp1 / rec_amp0: the wide margin with and without the
    gate; refined: {family: [numCtus, per CTU]}; vector_cost(mvx, mvy): of an integer vector)"""
    if "case" not in _CACHE:
        cur, ref = (p.astype(np.int64) for p in pictures())
        found = sw.PairSweep(oracle, cur, ref, 8, QP, sad=True, rmax=RANGE).records(RANGE)
        cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
        planes = mr.Planes(ref, 8, RANGE + 8)
        refined = {"nodes": mr.expected(oracle, cur_flat, 0, W, ref, W, H, 8, QP, found["nodes"], RANGE, planes=planes),
                   "pu": rp.expected(oracle, cur, ref, 8, QP, found["pu"], RANGE, "pu", planes=planes),
                   "small": rp.expected(oracle, cur, ref, 8, QP, found["small"], RANGE, "small", planes=planes)}
        default, amp1, amp0 = rules()
        rec, costs = sr.select(refined["nodes"][None], refined["pu"][None], refined["small"][None], W, H, rule=default)
        sl = mr.sqrt_lambda(oracle, QP, 8)
        _CACHE["case"] = dict(rec=rec[0], costs=costs[0], refined=refined, found=found,
                              rec_amp1=sr.select(refined["nodes"][None], refined["pu"][None], refined["small"][None], W, H, rule=amp1)[0][0],
                              rec_amp0=sr.select(refined["nodes"][None], refined["pu"][None], refined["small"][None], W, H, rule=amp0)[0][0],
                              vector_cost=lambda mvx, mvy: mr.qpel_cost(4 * mvx, 4 * mvy, sl))
    return _CACHE["case"]


def check_constructed(rec, costs, rec_amp1, rec_amp0, vector_cost):
    """what the three constructed CUs must show, on records [numCtus, 85] and costs [numCtus, 85, 8] of the default rule and on the records of the
    wide margin with (amp_mode 1) and without (amp_mode 0) the gate"""
    c, k = CU_2NxN
    assert rec["best"][c, k] == capi.PART_2NxN, costs[c, k]
    assert rec["cost_best"][c, k] == vector_cost(3, 0) + vector_cost(-2, 1), (costs[c, k], vector_cost(3, 0), vector_cost(-2, 1))
    c, k = CU_nLx2N
    assert rec["best"][c, k] == capi.PART_nLx2N, costs[c, k]
    assert rec["cost_best"][c, k] == vector_cost(1, 2) + vector_cost(4, 0)
    c, k = CU_Nx2N_16
    row = costs[c, k].astype(np.int64)
    assert row[2] < row[0] and row[2] <= row[1], ("Nx2N is not the best of the three symmetric sizes", row)
    assert min(row[4], row[5]) < row[0], ("no horizontal AMP split is cheaper than 2Nx2N", row)
    cheaper = 4 if row[4] <= row[5] else 5
    assert rec_amp1["avail"][c, k] & 0x30 == 0x30 and not rec_amp1["mask"][c, k] & 0x30, "amp_mode 1 must clear bits 4 and 5 behind Nx2N"
    assert rec_amp1["mask"][c, k] & 0xC0 == 0xC0
    assert rec_amp0["mask"][c, k] & (1 << cheaper)
