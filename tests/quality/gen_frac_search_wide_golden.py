"""tests/golden/ref_frac_search_wide.npz: what the REFERENCE's own TEncSearch::xPatternSearchFracDIF (Hadamard, half- then quarter-sample stage)
returns around integer vectors of up to +-64 samples for the 85 nodes, the 124 PUs and the 384 small PUs of five CTUs of the ragged 176 x 144
picture -- the file fhevc_motion_refine_pu_wide is pinned to (tests/test_oracle_golden_frac_wide.py without a GPU,
tests/test_gpu_motion_refine_pu_wide.py on one), and the first time the square refinement above +-8 meets the reference.  The layout is
tests/golden/ref_frac_search.npz's (tests/motion_golden.py: FracCase); picture, CTUs, entries and the calls into the reference are
oracle/gen_golden.py's (_pu_planes, _pu_blocks, _pu_search_case, _pu_family_counts, _pu_save), used as they are.

Cases (bit depth, QP, range, content):
  * the eight cases of tests/golden/ref_pattern_search_pu_wide.npz -- six pan cases, "white", "checker" -- on that file's planes, around that file's
    vectors (HM's own chain: xPatternSearch, then xPatternSearchFracDIF); no +-64 search is rerun;
  * two "blend" cases whose winners are mostly fractional at long vectors: the wide pan's current picture blended per 8x8 cell with itself one
    sample away (direction and weight drawn per cell), 8 bit and 10 bit with the low bits in use; integer vectors from the reference's
    xPatternSearch at R = 33 on the blended picture;
  * one "swing" case at 12 bit (samples 0 and 2^12 - 1) around random vectors of up to +-64: the clip of the interpolation works far from the CTU.
In every case every 7th entry is a seeded random vector in [-R, R] instead, in CTU 0 (-R, -R) and in CTU 8 (R, R): the window's own corners and
the replicated border are read.

CPU only; needs oracle/_ref (python __graft_entry__.py builds it where the reference's sources are).  Planes and integers only:

    python tests/quality/gen_frac_search_wide_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_golden as gg  # noqa: E402
import oracle_py as op  # noqa: E402

WIDE_SEARCH = os.path.join(ROOT, "tests", "golden", "ref_pattern_search_pu_wide.npz")
# (bit depth, QP, the case of the wide search file whose planes are blended): its pan moves 19 and 13 samples, inside the R = 33 of the rerun search
BLEND_CASES = ((8, 27, 0), (10, 22, 4))
BLEND_RANGE = 33
SWING_CASE = (12, 37, 64)
FAMILIES = (slice(0, 85), slice(85, 209), slice(209, 593))


def blend(cur, bd, seed):
    """the picture blended with itself one sample away, direction and weight drawn per 8x8 cell (gen_golden._pu_planes("blend"), on a given picture)"""
    rng = np.random.default_rng(seed)
    c = cur.astype(np.int64)
    p = np.pad(c, 1, mode="edge")
    cells = ((gg.PU_H + 7) // 8, (gg.PU_W + 7) // 8)
    dx, dy, wt = (rng.integers(lo, hi, size=cells).repeat(8, 0).repeat(8, 1)[:gg.PU_H, :gg.PU_W] for lo, hi in ((-1, 2), (-1, 2), (1, 3)))
    yy, xx = np.mgrid[0:gg.PU_H, 0:gg.PU_W]
    far = p[yy + 1 + dy, xx + 1 + dx]
    out = np.where(wt == 2, (c + far + 1) >> 1, (3 * c + far + 2) >> 2)
    assert 0 <= out.min() and out.max() < (1 << bd)
    return np.ascontiguousarray(out, np.int16)


def frac_case(ref, oracle, cur, refp, bd, qp, R, ints, seed, every=7):
    """xPatternSearchFracDIF around ints [5, 593, 2] (every `every`-th entry a random vector instead) -> (vin [5, 593, 2] int16, res [5, 593, 5] int32:
    satd_int, satd_best, cost_best, mvx, mvy; -1 = outside, half [n, 2] and quarter [n, 2] stage offsets and long [n] of the valid entries)"""
    rng = np.random.default_rng(seed)
    vin = np.zeros((len(gg.PU_CTUS), 593, 2), np.int16)
    res = np.full((len(gg.PU_CTUS), 593, 5), -1, np.int32)
    half, quarter, long_ = [], [], []
    for ci, c in enumerate(gg.PU_CTUS):
        where, blocks = gg._pu_blocks(c)
        v = ints[ci, where, :2].astype(np.int64)
        rnd = rng.integers(-R, R + 1, size=v.shape)
        if c == 0:
            rnd[:] = -R
        if c == 8:
            rnd[:] = R
        pick = np.array(where) % every == 0
        v[pick] = rnd[pick]
        assert np.abs(v).max() <= R
        b = np.ascontiguousarray(np.concatenate([blocks, v], axis=1), np.int32)
        o = np.zeros((len(where), 7), np.int32)
        assert ref.href_frac_search(cur.ctypes.data, refp.ctypes.data, gg.PU_W, gg.PU_W, gg.PU_H, bd, C.c_double(oracle.fho_lambda_intra(qp, bd)), len(where),
                                    b.reshape(-1), o.reshape(-1)) == len(where)
        vin[ci, where] = v
        res[ci, where] = o[:, [4, 3, 2, 0, 1]]    # satd_int, satd_best, cost_best, mvx, mvy: the library's record
        half.append(o[:, 5:7])
        quarter.append(o[:, :2] - 4 * v - 2 * o[:, 5:7])
        long_.append(np.abs(v).max(axis=1) > 8)
    return vin, res, np.concatenate(half), np.concatenate(quarter), np.concatenate(long_)


def main():
    ref, oracle = op.load_ref(), op.load_oracle()
    wide = np.load(WIDE_SEARCH)
    assert [int(v) for v in wide["size"]] == [gg.PU_W, gg.PU_H] and [int(c) for c in wide["ctus"]] == list(gg.PU_CTUS)
    pics, todo = [], []      # todo: (bd, qp, R, plane, integer vectors [5, 593, 2] or None = all random, is a pan case)

    def plane(cur, refp):
        pics.append((np.ascontiguousarray(cur, np.int16), np.ascontiguousarray(refp, np.int16)))
        return len(pics) - 1

    plane_of = {}
    for k, (bd, qp, R, p) in enumerate(tuple(int(v) for v in row) for row in wide["cases"]):
        if p not in plane_of:
            plane_of[p] = plane(wide[f"cur{p}"], wide[f"ref{p}"])
        pan = len(np.unique(wide[f"cur{p}"])) > 2
        todo.append((bd, qp, R, plane_of[p], wide[f"res{k}"][..., :2], pan))
    for bd, qp, k in BLEND_CASES:
        wbd, _, _, p = (int(v) for v in wide["cases"][k])
        assert wbd == bd
        cur = blend(wide[f"cur{p}"], bd, 800 + bd)
        assert bd == 8 or (cur & ((1 << (bd - 8)) - 1)).any()
        pl = plane(cur, wide[f"ref{p}"])
        ints = gg._pu_search_case(ref, oracle, *pics[pl], bd, qp, BLEND_RANGE)
        todo.append((bd, qp, BLEND_RANGE, pl, ints[..., :2], True))
    bd, qp, R = SWING_CASE
    todo.append((bd, qp, R, plane(*gg._pu_planes(bd, "swing")), None, False))

    out = {"size": np.array([gg.PU_W, gg.PU_H], np.int32), "ctus": np.array(gg.PU_CTUS, np.int32)}
    cases, counts = [], np.zeros(3, np.int64)
    half_wins, quarter_wins = np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64)     # among the entries with a long input vector
    for k, (bd, qp, R, p, ints, pan) in enumerate(todo):
        cur, refp = pics[p]
        every = 7 if ints is not None else 1
        vin, res, half, quarter, long_ = frac_case(ref, oracle, cur, refp, bd, qp, R, ints if ints is not None else np.zeros((5, 593, 2), np.int64), 2000 + k, every)
        np.add.at(half_wins, (half[long_, 1] + 1, half[long_, 0] + 1), 1)
        np.add.at(quarter_wins, (quarter[long_, 1] + 1, quarter[long_, 0] + 1), 1)
        valid = res[..., 2] != -1
        per_case = gg._pu_family_counts(valid)
        counts += per_case
        is_long = valid & (np.abs(vin.astype(np.int64)).max(axis=-1) > 8)
        longs = [int(is_long[:, s].sum()) for s in FAMILIES]
        frac = [int((is_long[:, s] & ((res[:, s, 3] & 3) | (res[:, s, 4] & 3)).astype(bool)).sum()) for s in FAMILIES]
        print(f"case {k}: bd {bd} qp {qp} R {R}: valid {per_case}, long input vectors per family {longs}, of them with a fractional winner {frac}")
        if pan:   # long vectors in every family of every pan case
            assert min(longs) > 0, (k, longs)
        out[f"in{k}"], out[f"out{k}"] = vin, res
        cases.append((bd, qp, R, p))
    # among the valid entries whose input vector has a component above 8, every candidate of both tables wins somewhere
    assert half_wins.all() and quarter_wins.all(), (half_wins, quarter_wins)
    for p, (cur, refp) in enumerate(pics):
        out[f"cur{p}"], out[f"ref{p}"] = cur, refp
    out["cases"], out["counts"] = np.array(cases, np.int32), counts.astype(np.int32)
    print("valid entries (nodes, PUs, small PUs):", counts.tolist(), "in", len(cases), "cases")
    print("among long input vectors: half-stage winners [dy + 1][dx + 1]:", half_wins.tolist(), "quarter-stage winners:", quarter_wins.tolist())
    gg._pu_save("ref_frac_search_wide.npz", out)


if __name__ == "__main__":
    main()
