"""Pins of tests/motion_pu_ref.py, the numpy restatement the GPU tests of the rectangular-PU motion search compare against (no GPU needed):
squares against the reference's own xPatternSearch (golden) and against the oracle in both distortions, the tile-sum form against the direct form
on every covered PU size at 10 bit, the tie rule, and the index map and geometries of include/fasthevc.h.

Not covered by any pin: a run of the reference's xPatternSearch on RECTANGLES (its harness searches square blocks only).  The rectangular shapes
rest on this restatement plus oracle.fho_satd, which is pinned to the reference's xGetHADs for non-square blocks."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_pu_ref as pr
from fasthevc_amd import capi, frames

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pattern_search.npz")
PU_SIZES = [(64, 32), (32, 64), (64, 16), (64, 48), (16, 64), (48, 64), (32, 16), (16, 32), (32, 8), (32, 24), (8, 32), (24, 32), (16, 8), (8, 16)]


def content(W, H, bd, seed):
    """two pictures [H, W] at bd bits with the low bits populated: a pan with overlaid noise"""
    ys = frames.pan_clip(W, H, 2, seed=seed)
    rng = np.random.default_rng(seed)
    return [(y.astype(np.int64) << (bd - 8)) + (rng.integers(0, 1 << (bd - 8), size=y.shape) if bd > 8 else 0) for y in ys]


def test_squares_equal_the_references_xPatternSearch(oracle):
    g = np.load(GOLDEN)
    W, H = 416, 240
    checked = 0
    for k, (bd, qp, rng, _seed) in enumerate(g["cases"]):
        stride = int(g[f"stride{k}"])
        pic = lambda flat: np.concatenate([flat, np.zeros(stride * H - flat.size, flat.dtype)]).reshape(H, stride)[:, :W].astype(np.int64)
        cur, ref = pic(g[f"cur{k}"]), pic(g[f"ref{k}"])
        costs = pr.mv_costs(oracle, int(rng), pr.sqrt_lambda(oracle, int(qp), int(bd)))
        for ci, c in enumerate(g[f"ctus{k}"][:3]):     # three CTUs per case: a corner, the interior / an edge
            cx, cy = int(c) % 7, int(c) // 7
            w, h = min(64, W - cx * 64), min(64, H - cy * 64)
            td = pr.tile_dists(cur, ref, int(rng), True, cx * 64, cy * 64, w, h)
            exp = g[f"nodes{k}"][ci]
            for node in range(85):
                x0, y0, n = pr.node_rect(node)
                if exp[node, 3] < 0:
                    assert x0 + n > w or y0 + n > h
                    continue
                r = pr.search_tiles(td, costs, int(rng), int(bd), x0, y0, n, n)
                assert (int(r["mvx"]), int(r["mvy"]), int(r["satd_best"]), int(r["cost_best"])) == tuple(int(v) for v in exp[node]), (k, c, node)
                checked += 1
    assert checked > 400


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("sad", [False, True])
def test_squares_equal_the_oracle_in_both_distortions(oracle, bd, sad):
    W, H, R, qp = 176, 144, 5, 30     # ragged: the last column 48 wide, the last row 16 tall
    cur, ref = content(W, H, bd, 3 + bd)[::-1]
    nodes, _ = pr.expected(oracle, cur, ref, bd, qp, R, sad)
    (cb, org, stride), (rb, _, _) = frames.to_pel_plane(np.zeros((H, W), np.uint8)), frames.to_pel_plane(np.zeros((H, W), np.uint8))
    m = frames.HM_MARGIN
    cb[m:m + H, m:m + W], rb[m:m + H, m:m + W] = cur, ref
    out = np.zeros(85, pr.DT)
    valid = 0
    for c in range(9):
        oracle.fho_motion_ctu_dist(C.c_void_p(cb.ctypes.data + 2 * org), stride, C.c_void_p(rb.ctypes.data + 2 * org), stride, W, H, c % 3, c // 3, bd, R,
                                   C.c_double(pr.sqrt_lambda(oracle, qp, bd)), 1 if sad else 0, C.c_void_p(out.ctypes.data))
        for name in pr.DT.names:
            assert np.array_equal(out[name], nodes[c][name]), (c, name)
        valid += int((out["cost_best"] != pr.MARKER).sum())
    assert valid == 4 * 85 + 2 * (2 + 12 + 48) + 2 * (4 + 16) + (3 + 12)   # whole CTUs; 48 x 64; 64 x 16; 48 x 16


@pytest.mark.parametrize("sad", [False, True])
def test_tile_sum_form_equals_the_direct_form_on_every_pu_size(oracle, sad):
    """10 bit: the sum of the tiles is shifted ONCE (a sum of shifted tile values would differ: asserted)"""
    W, H, R, bd, qp = 96, 80, 3, 10, 27
    cur, ref = content(W, H, bd, 11)[::-1]
    costs = pr.mv_costs(oracle, R, pr.sqrt_lambda(oracle, qp, bd))
    td = pr.tile_dists(cur, ref, R, sad)
    shifted_tiles_differ = False
    for i, (w, h) in enumerate(PU_SIZES):
        x0, y0 = (8 * i) % (W - w + 8), (16 * i) % (H - h + 8)    # at the picture's corner, inside, against its right and bottom edges
        fast = pr.search_tiles(td, costs, R, bd, x0, y0, w, h)
        direct = pr.search_direct(oracle, cur, ref, costs, R, bd, sad, x0, y0, w, h)
        assert fast == direct, ((w, h), fast, direct)
        wrong = (td[:, y0 // 8:(y0 + h) // 8, x0 // 8:(x0 + w) // 8] >> (bd - 8)).sum(axis=(1, 2))
        shifted_tiles_differ |= int(wrong[(2 * R + 1) ** 2 // 2]) != int(fast["satd_zero"])
    assert shifted_tiles_differ


def test_a_flat_pair_gives_the_first_raster_vector_of_least_vector_cost(oracle):
    W, H, R, bd, qp = 64, 64, 4, 8, 32
    flat = np.full((H, W), 77, np.int64)
    for sad in (False, True):
        nodes, pus = pr.expected(oracle, flat, flat, bd, qp, R, sad)
        costs = pr.mv_costs(oracle, R, pr.sqrt_lambda(oracle, qp, bd))
        m = int(np.argmin(costs))
        assert costs[m] == costs[(2 * R + 1) ** 2 // 2] and m == (2 * R + 1) ** 2 // 2   # the zero vector is the only cheapest one ...
        for a in (nodes, pus):
            assert (a["mvx"] == 0).all() and (a["mvy"] == 0).all() and (a["satd_best"] == 0).all() and (a["cost_best"] == costs[m]).all()
    # ... so take costs with a tie instead: every vector costs the same, the first in raster order (-R, -R) wins for every PU
    same = np.full((2 * R + 1) ** 2, 5, np.int64)
    td = pr.tile_dists(flat, flat, R, True)
    for k, s, p in pr.covered():
        r = pr.search_tiles(td, same, R, bd, *pr.pu_rect(k, s, p))
        assert (int(r["mvx"]), int(r["mvy"]), int(r["cost_best"])) == (-R, -R, 5)


def test_index_map_and_geometries():
    seen = {}
    for node in range(-1, 86):
        for shape in range(-1, 8):
            for part in range(-1, 3):
                i = capi.motion_pu_index(node, shape, part)
                assert i == pr.pu_index(node, shape, part)
                ok = part in (0, 1) and ((0 <= node < 5 and 0 <= shape < 6) or (5 <= node < 21 and 0 <= shape < 2))
                assert (i >= 0) == ok
                if ok:
                    seen[i] = (node, shape, part)
    assert sorted(seen) == list(range(capi.PUS_PER_CTU)) and capi.PUS_PER_CTU == pr.PUS_PER_CTU == 124
    assert [seen[i] for i in range(124)] == pr.covered()
    # the built library agrees where it is there
    if os.path.exists(capi.LIB_PATH):
        lib = capi.load_library()
        for node in range(-1, 86):
            for shape in range(-1, 8):
                for part in range(-1, 3):
                    assert lib.fhevc_motion_pu_index(node, shape, part) == pr.pu_index(node, shape, part)
    # geometries: the two parts tile the CU, part 0 first; sizes as the table of fasthevc.h
    sizes = set()
    for node, shape, part in pr.covered():
        nx, ny, s = pr.node_rect(node)
        (x0, y0, w0, h0), (x1, y1, w1, h1) = pr.pu_rect(node, shape, 0), pr.pu_rect(node, shape, 1)
        assert (x0, y0) == (nx, ny) and w0 * h0 + w1 * h1 == s * s and all(v % 8 == 0 for v in (x0, y0, w0, h0, x1, y1, w1, h1))
        if shape in (0, 2, 3):
            assert w0 == w1 == s and (x1, y1) == (nx, ny + h0) and h0 == (s // 2, 0, s // 4, 3 * s // 4)[shape]
        else:
            assert h0 == h1 == s and (x1, y1) == (nx + w0, ny) and w0 == (0, s // 2, 0, 0, s // 4, 3 * s // 4)[shape]
        sizes.add(pr.pu_rect(node, shape, part)[2:])
    assert sizes == set(PU_SIZES)
