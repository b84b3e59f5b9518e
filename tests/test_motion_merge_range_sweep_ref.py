"""Config 4 (P slices), without a GPU: the inputs of tests/test_gpu_motion_merge_range_sweep.py (tests/motion_merge_sweep_cases.py) probe what they are
meant to probe, at every max_range 1..64, every corner of the reach and bit depths 8, 10 and 12 -- computed from the CPU restatements alone
(motion_merge_ref, motion_merge_pu_ref, motion_skip_ref, each pinned by its own test) --, and the index arithmetic of refine_stage_window_reach
(k_refine_tile.h), restated in numpy, stages every window cell that refine_tile_diff reads for its value and, in rows, not one more."""
import os
import re

import numpy as np
import pytest

import motion_merge_ref as mg
import motion_merge_sweep_cases as cs
import motion_refine_ref as mr
import motion_skip_ref as sk

BLOCKS = [tuple(range(lo, lo + 4)) for lo in range(1, 65, 4)]
block_id = lambda b: f"R{b[0]}-{b[-1]}"
# what the 168 x 152 picture gives: entries that inherit, of the valid ones, per family and level
COUNTS = {("nodes", 0): (3, 4), ("nodes", 1): (19, 20), ("nodes", 2): (89, 90), ("nodes", 3): (398, 399), ("pu", 0): (30, 48), ("pu", 1): (207, 240),
          ("pu", 2): (339, 360), ("small", 2): (678, 720), ("small", 3): (1554, 1596)}


# ---- the corner pairs ---------------------------------------------------------------------------------------------------------------------------------------

def test_the_picture_feeds_every_level_of_every_family():
    counts = cs.level_counts()
    assert counts == COUNTS
    for (fam, lvl), (fed, valid) in counts.items():
        if fam == "nodes":
            assert fed >= 3 if lvl == 0 else 4 * fed >= 3 * valid, (fam, lvl, fed, valid)
        else:
            assert 2 * fed >= valid, (fam, lvl, fed, valid)
    # for each sign of a corner, an entry that inherits lies on the side of its CTU that the sign points to, on every level of every family
    for fam, (valid, fed) in cs.geometry().items():
        levels = np.array([cs.level_of(fam, e) for e in range(valid.shape[1])])
        for sx, sy in cs.CORNERS:
            side = np.array([cs.on_the_side(fam, e, sx, sy) for e in range(valid.shape[1])])
            for lvl in set(levels.tolist()):
                assert fed[:, side & (levels == lvl)].any(), (fam, lvl, sx, sy)


@pytest.mark.parametrize("block", BLOCKS, ids=block_id)
@pytest.mark.parametrize("bd", cs.BIT_DEPTHS)
def test_corner_pairs_win_with_q_at_no_distortion(oracle, bd, block):
    """check_corner holds the restatements' records against the closed form on every entry that geometry() says inherits: the winners are exactly those,
    so the shares and sides asserted above are the shares and sides of the winners.  On unrelated noise the same records leave coefficients on every
    valid node: the skip stage is a probe of every sample"""
    for R in block:
        case = cs.corner_case(oracle, bd, R)
        assert case["c1"] > 0
        other = cs.noise("unrelated", "sweep", bd, R)
        planes = mr.Planes(case["ref"], bd, cs.PAD)
        for corner in cs.CORNERS:
            c = case["corners"][corner]
            assert c["q"] == (corner[0] * (4 * R + 3), corner[1] * (4 * R + 3))
            n = cs.check_corner(c["exp"], c["q"], case["c1"])
            assert n == {"nodes": 509, "pu": 576, "small": 2232, "skip": 509}, (bd, R, corner, n)
            for fam in ("nodes", "pu", "small"):
                won = (c["exp"][fam]["satd_best"] == 0) & (c["exp"][fam]["mvx"] == c["q"][0]) & (c["exp"][fam]["mvy"] == c["q"][1])
                assert np.array_equal(won, cs.geometry()[fam][1]), (bd, R, corner, fam)
            unrelated = sk.expected(other, case["ref"], cs.W, cs.H, bd, cs.SKIP_QP, c["exp"]["nodes"], R, planes=planes)
            valid = cs.geometry()["nodes"][0]
            assert (unrelated["coef_max"][valid] > 0).all() and (unrelated["coef_max"][valid] != sk.MARK).all(), (bd, R, corner)


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", BLOCKS, ids=block_id)
def test_the_draw_holds_every_list_and_every_edge_of_the_reach(block):
    for R in block:
        refined, reach = cs.draw_refined(R), 4 * R + 3
        for fam in ("nodes", "pu", "small"):
            lengths, pairs = cs.draw_statistics(refined, R, fam)
            assert lengths == {1, 2, 3, 4, 5}, (R, fam, lengths)
            assert all(fired > 0 and passed > 0 for fired, passed in pairs.values()), (R, fam, pairs)
        ok = refined["cost_best"] != mg.MARK
        x, y = refined["mvx"].astype(np.int64), refined["mvy"].astype(np.int64)
        within = ok & (np.abs(x) <= reach) & (np.abs(y) <= reach)
        for name, hit in (("x+", x == reach), ("x-", x == -reach), ("y+", y == reach), ("y-", y == -reach)):
            assert int((within & hit).sum()) >= 8, (R, name)
        assert int((ok & ((x == reach + 1) | (y == reach + 1))).sum()) >= 8 and int((ok & ((x == -reach - 1) | (y == -reach - 1))).sum()) >= 8, R
        # the second set of skip inputs: vectors on the limit in both signs on both axes, markers, and records one quarter sample beyond
        m = cs.random_merge(np.random.default_rng([78, R]), (cs.N, 85), R)
        mok = m["cost_best"] != mg.MARK
        mx, my = m["mvx"].astype(np.int64), m["mvy"].astype(np.int64)
        for hit in (mx == reach, mx == -reach, my == reach, my == -reach):
            assert (mok & hit & (np.abs(mx) <= reach) & (np.abs(my) <= reach)).any(), R
        assert (~mok).any() and (mok & ((np.abs(mx) == reach + 1) | (np.abs(my) == reach + 1))).any(), R


def test_the_existing_draw_is_unchanged():
    """motion_merge_pu_ref.random_refined without a pool draws what it drew before it took one"""
    import motion_merge_pu_ref as mpu
    a = mpu.random_refined(np.random.default_rng(77), (12, 85), 8)
    b = mpu.random_refined(np.random.default_rng(77), (12, 85), 8, pool=[(-5, 2), (3, 3), (35, -35), (0, -7)])
    assert a.tobytes() == b.tobytes()
    assert set(zip(a["mvx"][np.abs(a["mvx"]) <= 35].tolist(), a["mvy"][np.abs(a["mvx"]) <= 35].tolist())) >= {(-5, 2), (3, 3), (35, -35), (0, -7)}


def test_no_two_pictures_share_a_seed():
    seeds = set()
    for kind in cs.KINDS:
        for variant in cs.VARIANTS:
            for bd in cs.BIT_DEPTHS:
                for R in cs.RANGES:
                    for extra in (0, 1):
                        seeds.add(tuple(cs.seed(kind, variant, bd, R, extra)))
    assert len(seeds) == len(cs.KINDS) * len(cs.VARIANTS) * 3 * 64 * 2
    a, b = cs.noise("corner", "sweep", 8, 5), cs.noise("corner", "guarded", 8, 5)
    assert (a != b).mean() > 0.9


# ---- refine_stage_window_reach's index arithmetic against what refine_tile_diff reads for its value ------------------------------------------------------------

def kernel_taps():
    """kLumaTaps of k_refine_tile.h -> {fraction: eight coefficients over samples x - 3 .. x + 4}"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fasthevc_amd", "csrc", "k_refine_tile.h")
    text = open(path).read()
    body = text[text.index("kLumaTaps[16]"):]
    pairs = re.findall(r"FHEVC_PK\(\s*(-?\d+)\s*,\s*(-?\d+)\s*\)", body[:body.index("};")])
    assert len(pairs) == 16
    flat = [int(v) for p in pairs for v in p]
    return {f: tuple(flat[8 * f:8 * f + 8]) for f in range(4)}


def test_the_kernel_taps_are_the_restatements():
    taps = kernel_taps()
    assert taps[0] == (0, 0, 0, 64, 0, 0, 0, 0)
    assert all(taps[f] == tuple(mr.TAPS[f]) for f in (1, 2, 3))


@pytest.mark.parametrize("MR", [8, 64])
def test_the_staged_part_holds_every_cell_read_for_its_value_and_no_row_more(MR):
    """the claim of the comment above refine_stage_window_reach: rows and columns MR - R .. RP - 1 - (MR - R) hold every sample that a vector within the
    reach of R reads for its value; the rows are exactly those, the columns those widened to whole 4-sample chunks.  -(4R + 3) reads the first of them
    and +(4R + 3) the last (as do -+(4R + 2), the half-sample filter having eight taps) -- +-(4R + 1) and +-4R do not, their outer tap being 0: they cannot
    show a missing row or column"""
    taps = kernel_taps()
    RP = 64 + 2 * MR + 8
    for R in range(1, MR + 1):
        rows, cols = cs.staged_part(MR, R)
        skip, reach = MR - R, 4 * R + 3
        assert rows[0] >= 0 and rows[-1] <= RP - 1 and cols[0] >= 0 and cols[-1] <= RP - 1                  # inside the window
        assert np.array_equal(rows, np.arange(skip, RP - skip))                                             # contiguous, symmetric
        assert np.array_equal(cols, np.arange(cols[0], cols[-1] + 1)) and cols[0] % 4 == 0 and (cols[-1] + 1) % 4 == 0
        lo, hi = RP, -1
        for q in range(-reach, reach + 1):
            read = cs.read_for_value(MR, q, taps)
            assert rows[0] <= read[0] and read[-1] <= rows[-1], (MR, R, q, "rows")                         # containment; each axis reads the same set
            assert cols[0] <= read[0] and read[-1] <= cols[-1], (MR, R, q, "columns")
            lo, hi = min(lo, int(read[0])), max(hi, int(read[-1]))
            if abs(q) < reach - 1:
                assert read[0] > skip and read[-1] < RP - 1 - skip, (MR, R, q)                              # only the last two magnitudes touch the ends
        assert cs.read_for_value(MR, -reach, taps)[0] == rows[0] == lo and cs.read_for_value(MR, reach, taps)[-1] == rows[-1] == hi    # tight rows
        assert 0 <= lo - cols[0] <= 3 and 0 <= cols[-1] - hi <= 3 and lo - cols[0] == skip % 4 == cols[-1] - hi                          # chunk widening only
        # a first chunk rounded up instead of down loses cells that are read exactly where skip is no multiple of 4
        assert (4 * ((skip + 3) >> 2) > lo) == (skip % 4 != 0)
