"""Pins of tests/motion_pu_small_ref.py, the numpy restatement the GPU tests of the motion search of the 4-sample PUs compare against (no GPU
needed): the quadrant form against the direct form (oracle.fho_satd on the whole block, pinned to the reference's xGetHADs on its 4x4 branch) for
all six PU sizes, both distortions, 8 / 10 / 12 bit; the trap of the three-quarter parts; additivity in SAD mode; the tie rule; the index map.

Not covered by any pin: a run of the reference's xPatternSearch on these PUs (its harness searches square blocks only)."""
import os

import numpy as np
import pytest

import motion_pu_ref as pr
import motion_pu_small_ref as ps
from fasthevc_amd import capi, frames

PU_SIZES = [(16, 4), (16, 12), (4, 16), (12, 16), (8, 4), (4, 8)]


def content(W, H, bd, seed):
    """two pictures [H, W] at bd bits with the low bits populated: a pan with overlaid noise"""
    ys = frames.pan_clip(W, H, 2, seed=seed)
    rng = np.random.default_rng(seed)
    return [(y.astype(np.int64) << (bd - 8)) + (rng.integers(0, 1 << (bd - 8), size=y.shape) if bd > 8 else 0) for y in ys]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("sad", [False, True], ids=["satd", "sad"])
def test_quadrant_form_equals_the_direct_form_on_every_pu_size(oracle, sad, bd):
    """above 8 bit the sum of the quadrants is shifted ONCE (a sum of shifted quadrants would differ: asserted)"""
    W, H, R, qp = 48, 40, 2, 27
    cur, ref = content(W, H, bd, 11 + bd)[::-1]
    costs = pr.mv_costs(oracle, R, pr.sqrt_lambda(oracle, qp, bd))
    qd = ps.quad_dists(cur, ref, R, sad)
    shifted_quads_differ = False
    for i, (w, h) in enumerate(PU_SIZES):
        for x0, y0 in ((0, 0), (4 * (i + 1), 4 * (i % 3 + 1)), (W - w, H - h)):    # the picture's corner, inside, against its right and bottom edges
            fast = ps.search_quads(qd, costs, R, bd, x0, y0, w, h)
            direct = pr.search_direct(oracle, cur, ref, costs, R, bd, sad, x0, y0, w, h)
            assert fast == direct, ((w, h), (x0, y0), fast, direct)
            wrong = (qd[:, y0 // 4:(y0 + h) // 4, x0 // 4:(x0 + w) // 4] >> (bd - 8)).sum(axis=(1, 2))
            shifted_quads_differ |= int(wrong[(2 * R + 1) ** 2 // 2]) != int(fast["satd_zero"])
    assert shifted_quads_differ == (bd > 8)


def test_three_quarter_part_is_not_the_nodes_satd_minus_the_quarter(oracle):
    """the node's SATD is built from 8x8 Hadamards, the three-quarter part from 4x4 ones: on this content the shortcut is wrong"""
    W, H, R, bd = 64, 64, 2, 8
    cur, ref = content(W, H, bd, 7)[::-1]
    qd, td = ps.quad_dists(cur, ref, R, False), pr.tile_dists(cur, ref, R, False)
    differ = total = 0
    for k in range(5, 21):
        x0, y0, n = pr.node_rect(k)
        node8 = td[:, y0 // 8:(y0 + n) // 8, x0 // 8:(x0 + n) // 8].sum(axis=(1, 2))   # what fhevc_motion_search computes for the node
        node4 = ps.quad_sum(qd, bd, x0, y0, n, n)
        for shape in range(2, 6):
            quarter = 0 if shape in (2, 4) else 1
            q = ps.quad_sum(qd, bd, *pr.pu_rect(k, shape, quarter))
            big = ps.quad_sum(qd, bd, *pr.pu_rect(k, shape, 1 - quarter))
            assert np.array_equal(big, node4 - q)        # the sixteen 4x4 Hadamards minus the quarter's four
            differ += int((big != node8 - q).sum())
            total += big.size
    assert differ > 0, (differ, total)


def test_sad_parts_sum_to_the_nodes_sad_at_every_vector(oracle):
    W, H, R, bd = 64, 64, 3, 8
    cur, ref = content(W, H, bd, 5)[::-1]
    qd, td = ps.quad_dists(cur, ref, R, True), pr.tile_dists(cur, ref, R, True)
    for k in range(5, 85):
        x0, y0, n = pr.node_rect(k)
        node = td[:, y0 // 8:(y0 + n) // 8, x0 // 8:(x0 + n) // 8].sum(axis=(1, 2))
        for shape in (range(2, 6) if k < 21 else range(2)):
            parts = [ps.quad_sum(qd, bd, *pr.pu_rect(k, shape, p)) for p in (0, 1)]
            assert np.array_equal(parts[0] + parts[1], node), (k, shape)


def test_a_flat_pair_gives_the_zero_vector(oracle):
    W, H, R, bd, qp = 64, 64, 4, 8, 32
    flat = np.full((H, W), 77, np.int64)
    costs = pr.mv_costs(oracle, R, pr.sqrt_lambda(oracle, qp, bd))
    centre = (2 * R + 1) ** 2 // 2
    assert int(np.argmin(costs)) == centre and (costs[np.arange(costs.size) != centre] > costs[centre]).all()
    for sad in (False, True):
        pus = ps.expected(oracle, flat, flat, bd, qp, R, sad)
        assert (pus["mvx"] == 0).all() and (pus["mvy"] == 0).all() and (pus["satd_best"] == 0).all() and (pus["cost_best"] == costs[centre]).all()
    # with a tie between all vectors the first in raster order, (-R, -R), wins for every PU
    same = np.full((2 * R + 1) ** 2, 5, np.int64)
    qd = ps.quad_dists(flat, flat, R, True)
    for k, s, p in ps.covered():
        r = ps.search_quads(qd, same, R, bd, *pr.pu_rect(k, s, p))
        assert (int(r["mvx"]), int(r["mvy"]), int(r["cost_best"])) == (-R, -R, 5)


def test_index_map_and_geometries():
    seen = {}
    for node in range(-1, 87):
        for shape in range(-1, 8):
            for part in range(-1, 3):
                i = capi.motion_pu_small_index(node, shape, part)
                assert i == ps.pu_small_index(node, shape, part)
                ok = part in (0, 1) and ((5 <= node < 21 and 2 <= shape < 6) or (21 <= node < 85 and 0 <= shape < 2))
                assert (i >= 0) == ok and (ok or i == -1)
                if ok:
                    assert i not in seen
                    seen[i] = (node, shape, part)
    assert sorted(seen) == list(range(384)) and capi.PUS_SMALL_PER_CTU == ps.PUS_SMALL_PER_CTU == 384
    assert [seen[i] for i in range(384)] == ps.covered()
    # the built library agrees where it is there
    if os.path.exists(capi.LIB_PATH):
        lib = capi.load_library()
        for node in range(-1, 87):
            for shape in range(-1, 8):
                for part in range(-1, 3):
                    assert lib.fhevc_motion_pu_small_index(node, shape, part) == ps.pu_small_index(node, shape, part)
    # geometries: the two parts tile the CU; every covered PU has a side that is no multiple of 8; the six sizes of fasthevc.h
    sizes = set()
    for node, shape, part in ps.covered():
        s = pr.node_rect(node)[2]
        (_, _, w0, h0), (_, _, w1, h1) = pr.pu_rect(node, shape, 0), pr.pu_rect(node, shape, 1)
        assert w0 * h0 + w1 * h1 == s * s
        w, h = pr.pu_rect(node, shape, part)[2:]
        assert w % 4 == 0 and h % 4 == 0 and (w % 8 or h % 8)
        sizes.add((w, h))
    assert sizes == set(PU_SIZES)
