"""tests/pu_shape_ref.py (the numpy restatement of the partition-size selection) against hand-computed cases: a handful of entries set by hand,
everything else the marker.  No GPU.  The last test confirms, on the CPU restatements of the searches and refinements, the three constructed CUs
that tests/test_gpu_pu_shape.py expects of the real pipeline."""
import numpy as np
import pytest

import pu_shape_ref as sr
from fasthevc_amd import capi

M = sr.MARKER


def empty():
    """cost_best of one CTU's entries, all the marker"""
    return np.full(85, M, np.uint32), np.full(124, M, np.uint32), np.full(384, M, np.uint32)


def rule(q8=0, ab=0, amp=1):
    return capi.pu_shape_rule(q8, ab, amp)


# one node per level: the CTU, the last 32x32, a 16x16 in the middle, an 8x8 in the middle
LEVEL_NODES = [(0, 0), (1, 4), (2, 11), (3, 50)]


@pytest.mark.parametrize("lvl,k", LEVEL_NODES)
@pytest.mark.parametrize("p", [1, 2, 4, 5, 6, 7])
def test_index_formulas_per_level_and_partition_size(lvl, k, p):
    """the two parts of partition size p of node k are read where fhevc_motion_pu_index / fhevc_motion_pu_small_index put them"""
    assert sr.level(k) == lvl
    shape = p - 1 if p <= 2 else p - 2
    in_pu = [capi.motion_pu_index(k, shape, part) for part in (0, 1)]
    in_small = [capi.motion_pu_small_index(k, shape, part) for part in (0, 1)]
    nodes, pus, small = empty()
    nodes[k] = 1000
    if lvl == 3 and p >= 4:
        assert in_pu == [-1, -1] and in_small == [-1, -1] and sr.parts(k, p) is None
        pus[:], small[:] = 7, 7          # whatever the entries hold, AMP of an 8x8 CU stays unavailable
        rec, costs = sr.select_ctu(nodes, pus, small, 64, 64)
        assert costs[k, p] == M and not rec["avail"][k] & (1 << p)
        return
    assert (in_pu[0] >= 0) != (in_small[0] >= 0), "exactly one family covers the combination"
    fam, src, idx = ("pu", pus, in_pu) if in_pu[0] >= 0 else ("small", small, in_small)
    assert sr.parts(k, p) == (fam, idx[0], idx[1])
    src[idx[0]], src[idx[1]] = 300, 45
    rec, costs = sr.select_ctu(nodes, pus, small, 64, 64)
    row = [M] * 8
    row[0], row[p] = 1000, 345
    assert costs[k].tolist() == row
    # default rule: margins 0 leave the best size and the 2Nx2N that HM always checks; the AMP gate keeps both pairs behind b3 = 0
    assert tuple(rec[k]) == (1000, 345, 1000, p, 0, (1 << p) | 1, (1 << p) | 1)
    # every other node: only its own (marker) entries
    others = np.delete(np.arange(85), k)
    assert (costs[others] == M).all() and (rec["best"][others] == 255).all() and (rec["mask"][others] == 1).all() and (rec["avail"][others] == 0).all()
    # without the small PUs everything taken from them is unavailable
    rec0, costs0 = sr.select_ctu(nodes, pus, None, 64, 64)
    assert costs0[k, p] == (345 if fam == "pu" else M)


def set_pair(pus, small, k, p, a, b):
    fam, e0, e1 = sr.parts(k, p)
    src = pus if fam == "pu" else small
    src[e0], src[e1] = a, b


def test_tie_order():
    nodes, pus, small = empty()
    k = 2
    nodes[k] = 500
    set_pair(pus, small, k, 1, 100, 100)     # 2NxN 200
    set_pair(pus, small, k, 2, 150, 50)      # Nx2N 200: checked first
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64)
    assert (rec["best"][k], rec["second"][k], rec["cost_best"][k], rec["cost_second"][k]) == (2, 1, 200, 200)
    assert rec["mask"][k] == 0b111 and rec["avail"][k] == 0b111        # margins 0: the two that tie, and 2Nx2N always
    # 2Nx2N equal to everything: best 0, second Nx2N
    nodes[k] = 200
    for p in (4, 5, 6, 7):
        set_pair(pus, small, k, p, 199, 1)
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64)
    assert (rec["best"][k], rec["second"][k], rec["cost_best"][k], rec["cost_second"][k]) == (0, 2, 200, 200)
    assert rec["mask"][k] == 0b11110111 and rec["avail"][k] == 0b11110111


def test_saturation_and_marker_parts():
    nodes, pus, small = empty()
    k = 7
    nodes[k] = M                                  # inside the picture, but the refinement marked it (vector beyond max_range)
    set_pair(pus, small, k, 1, 0xFFFFFFF0, 0xFFFFFFF0)
    set_pair(pus, small, k, 2, 0xFFFFFFF0, M)      # a marker in one part: unavailable
    set_pair(pus, small, k, 6, M, 3)
    rec, costs = sr.select_ctu(nodes, pus, small, 64, 64)
    assert costs[k].tolist() == [M, 0xFFFFFFFE, M, M, M, M, M, M]
    assert tuple(rec[k]) == (M, 0xFFFFFFFE, M, 1, 255, 0b11, 0b10)          # the saturated sum is available; bit 0 of the mask is set all the same
    # nothing available at all inside the picture: still mask & 1
    assert tuple(rec[8]) == (M, M, M, 255, 255, 1, 0)


def test_margin_arithmetic_near_2_32_does_not_wrap():
    nodes, pus, small = empty()
    k = 0
    nodes[k] = 0xFFFFFF00
    set_pair(pus, small, k, 1, 0xFFFFFFF0, 0xFFFFFFF0)      # 0xFFFFFFFE
    set_pair(pus, small, k, 2, 0x7FFFFFFF, 0x7FFFFFFF)      # 0xFFFFFFFE as well
    # limit = 0xFFFFFF00 + 0 + (0xFFFFFF00 * 65535 >> 8) is far above 2^32: in 32 bits it would wrap below cost_best and drop both
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64, rule(65535, 0, 0))
    assert rec["best"][k] == 0 and rec["mask"][k] == 0b111
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64, rule(0, 0xFD, 0))
    assert rec["mask"][k] == 0b001                                       # 0xFFFFFF00 + 0xFD < 0xFFFFFFFE
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64, rule(0, 0xFE, 0))
    assert rec["mask"][k] == 0b111
    # the relative margin is floored: cost_best 1000, q8 = 13 -> limit 1000 + 50
    nodes[k] = 1000
    set_pair(pus, small, k, 1, 1000, 50)
    set_pair(pus, small, k, 2, 1000, 51)
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64, rule(13, 0, 0))
    assert rec["mask"][k] == 0b011
    # margins are per level: the same costs at a 32x32 node with the margin given to level 0 only
    nodes[1] = 1000
    set_pair(pus, small, 1, 1, 1000, 50)
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64, rule([13, 0, 0, 0], 0, 0))
    assert rec["mask"][0] == 0b011 and rec["mask"][1] == 0b001


@pytest.mark.parametrize("c0,c2,c1,kept", [(100, 200, 300, 0xF0), (300, 100, 200, 0xC0), (300, 200, 100, 0x30), (M, M, M, 0x00),
                                           (M, 100, 100, 0xC0), (100, 100, 100, 0xF0)])
def test_amp_gate(c0, c2, c1, kept):
    """b3 = 0 keeps both AMP pairs, 2 (Nx2N) the vertical pair (bits 6, 7), 1 (2NxN) the horizontal pair (bits 4, 5), none available: no AMP"""
    nodes, pus, small = empty()
    k = 12      # a 16x16 node: its AMP parts come from the small PUs
    nodes[k] = c0
    half = lambda c: (M, M) if c == M else (c - 1, 1)
    set_pair(pus, small, k, 2, *half(c2))
    set_pair(pus, small, k, 1, *half(c1))
    for p in (4, 5, 6, 7):
        set_pair(pus, small, k, p, 5, 5)          # every AMP size is the cheapest by far
    big = rule(0, 0x7FFFFFFF, 1)
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64, big)
    three = sum(1 << p for p, c in ((0, c0), (1, c1), (2, c2)) if c != M)
    assert rec["best"][k] == 4 and rec["avail"][k] == 0xF0 | three
    assert rec["mask"][k] == (kept | three | 1)
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64, rule(0, 0x7FFFFFFF, 0))
    assert rec["mask"][k] == (0xF0 | three | 1)          # amp_mode 0: no gate
    # the gate only clears: with margins 0 the four AMP sizes tie for the best, and what b3 does not allow is not offered all the same
    rec, _ = sr.select_ctu(nodes, pus, small, 64, 64, rule(0, 0, 1))
    assert rec["mask"][k] == (1 | (kept & 0xF0))


def test_invalid_nodes_and_levels_at_the_edge():
    """valid 40 x 8: only the 8x8 nodes 21..25 lie wholly inside; valid 40 x 40: nodes of three levels do"""
    nodes, pus, small = (np.full(n, 10, np.uint32) for n in (85, 124, 384))
    rec, costs = sr.select_ctu(nodes, pus, small, 40, 8)
    inside = [21, 22, 23, 24, 25]
    for k in range(85):
        if k in inside:
            assert tuple(rec[k]) == (10, 10, 20, 0, 2, 1, 0b111) and costs[k].tolist() == [10, 20, 20, M, M, M, M, M]
        else:
            assert tuple(rec[k]) == (M, M, M, 255, 255, 0, 0) and (costs[k] == M).all()
    rec, _ = sr.select_ctu(nodes, pus, small, 40, 40)
    valid = [k for k in range(85) if sr.node_rect(k)[0] + sr.node_rect(k)[2] <= 40 and sr.node_rect(k)[1] + sr.node_rect(k)[2] <= 40]
    assert 1 in valid and 0 not in valid and 2 not in valid and sorted(k for k in range(85) if rec["avail"][k]) == valid


def test_select_over_a_band_uses_the_picture_geometry():
    """200 x 136 (4 x 3 CTUs, ragged by 8 on both sides), rows 1..2: the last column and row hold the edge-crossing nodes"""
    W, H = 200, 136
    rng = np.random.default_rng(5)
    nodes, pus, small = sr.random_entries(rng, 2, 8)
    rec, costs = sr.select(nodes, pus, small, W, H, rows=(1, 3))
    assert rec.shape == (2, 8, 85) and costs.shape == (2, 8, 85, 8)
    one, c1 = sr.select_ctu(nodes["cost_best"][1, 7], pus["cost_best"][1, 7], small["cost_best"][1, 7], 8, 8)       # the corner CTU
    sr.same(rec[1, 7], one)
    assert np.array_equal(costs[1, 7], c1) and rec["avail"][1, 7, 21] and not rec["avail"][1, 7, 22] and not rec["avail"][1, 7, 0]
    full, _ = sr.select_ctu(nodes["cost_best"][0, 0], pus["cost_best"][0, 0], small["cost_best"][0, 0], 64, 64)         # row 1, column 0: whole
    sr.same(rec[0, 0], full)
    # the drawn fields make the cases occur: ties, saturated sums, markers, nothing available
    assert (costs == sr.SATURATED).any() and (rec["best"] == 255).any() and (rec["cost_best"] == rec["cost_second"]).any()


# ---- the three constructed CUs of the GPU test's real pipeline, confirmed on the CPU restatements ----------------------------------------------------

def test_constructed_motions_give_the_expected_partition_sizes(oracle):
    """SAD searches at range 8, quarter-sample refinements and the selection, all on the CPU restatements, over the pair of pu_shape_cases"""
    import pu_shape_cases as pc
    case = pc.constructed_case(oracle)
    pc.check_constructed(case["rec"], case["costs"], case["rec_amp1"], case["rec_amp0"], case["vector_cost"])
    # both parts of the winning sizes refine to SATD 0 at their integer vectors
    pu = case["refined"]["pu"]
    for (c, k), shape, vectors in ((pc.CU_2NxN, 0, ((3, 0), (-2, 1))), (pc.CU_nLx2N, 4, ((1, 2), (4, 0)))):
        for part, (vx, vy) in enumerate(vectors):
            e = pu[c, capi.motion_pu_index(k, shape, part)]
            assert (e["satd_best"], e["mvx"], e["mvy"]) == (0, 4 * vx, 4 * vy)
    # the pair is not trivial elsewhere: several sizes win somewhere, and the ragged CTUs carry invalid nodes
    assert len(set(case["rec"]["best"].reshape(-1).tolist())) >= 5 and (case["rec"]["best"][3] == 255).any()
