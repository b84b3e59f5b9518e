"""tests/golden/ref_motion_centred.npz: what the REFERENCE's own xPatternSearch and xPatternSearchFracDIF return for a search and a refinement around a
centre P with the predictor 4 P -- the file fhevc_motion_search_pu_centred and fhevc_motion_refine_pu_centred are pinned to
(tests/test_motion_centred_ref.py without a GPU, tests/test_gpu_motion_centred.py on one).

A search around P with predictor 4 P on plane `ref` IS the reference's zero-predictor search on ref'(x, y) = ref(clamp(x + Px), clamp(y + Py)): the
same candidates, the same distortions, and the bits of v - P where the reference counts the bits of v' = v - P.  Its vectors come out shifted by P
(v = v' + P, q = q' + 4 P).  HM clamps in ref' coordinates, the library in ref coordinates, so the two agree only for entries whose every read stays
inside the picture in BOTH coordinate systems (position s in ref' and position s + P in ref): the block at any d of the window (`inside`), and 4 more
samples each way for the refinement's taps (`inside_frac`).  Tests compare
the flagged entries only and assert their number per family and case against `counts` / `counts_frac`.  In every case all valid entries of CTU 4 are
flagged (asserted here): its centres keep the window and the taps inside the picture.

Picture, CTUs, entries and the calls into the reference are oracle/gen_golden.py's (PU_W, PU_H, PU_CTUS, _pu_blocks), used as they are; only
href_pattern_search_rect and href_frac_search are called.  Cases: 8 / 10 / 12 bit, QPs 0 / 32 / 51, R 1 / 5 / 8, each value with each of the others'
once; centres that are the content's true pan ((20, -12) and (-24, 4): `A`, `B`), the extremes (+-56, -+56) (`C`, CTU 4 at the pan), a different
centre per CTU with the window's first column on each of the 8 residues (`D`, `E`).  The refinement runs around the file's own integer vectors; every
7th entry is a seeded random vector of the window instead.

CPU only; needs oracle/_ref (python __graft_entry__.py builds it where the reference's sources are).  Planes and integers only:

    python tests/quality/gen_motion_centred_golden.py
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
from fasthevc_amd import frames  # noqa: E402

PANS = ((20, -12), (-24, 4))          # content p: the current picture is the reference displaced by PANS[p], plus noise
Z = (0, 0)
CENTRES = {
    "A": [PANS[0]] * 9,
    "B": [PANS[1]] * 9,
    "C": [(-56, 56), Z, (56, -56), Z, PANS[0], Z, (56, 56), Z, (-56, -56)],
    "D": [(1, -3), Z, (2, 5), Z, (3, -7), Z, (4, 2), Z, (5, -1)],
    "E": [(6, 1), Z, (7, -2), Z, (-8, 0), Z, (-3, 3), Z, (16, -4)],
}
# (bit depth, QP, range, content, centre set)
CASES = ((8, 0, 1, 0, "A"), (8, 32, 5, 1, "B"), (8, 51, 8, 0, "C"), (10, 0, 5, 0, "D"), (10, 32, 8, 1, "E"), (10, 51, 1, 0, "C"), (12, 0, 8, 1, "B"),
         (12, 32, 1, 0, "E"), (12, 51, 5, 1, "D"))
TAPS = 4


def planes(bd, p):
    """-> (cur, ref) int16 [H, W]: cur(x, y) = ref(clamp(x + vx), clamp(y + vy)) + noise of a few levels, the low bits in use above 8 bit"""
    rng = np.random.default_rng(300 + 10 * bd + p)
    ref = frames.pan_clip(gg.PU_W, gg.PU_H, 1, seed=80 + p)[0].astype(np.int64) << (bd - 8)
    if bd > 8:
        ref = ref + rng.integers(0, 1 << (bd - 8), size=ref.shape)
    cur = displaced(ref, *PANS[p]) + rng.integers(-(2 << (bd - 8)), (2 << (bd - 8)) + 1, size=ref.shape)
    return np.ascontiguousarray(np.clip(cur, 0, (1 << bd) - 1), np.int16), np.ascontiguousarray(ref, np.int16)


def displaced(ref, px, py):
    """ref'(x, y) = ref(clamp(x + px), clamp(y + py))"""
    h, w = ref.shape
    yy = np.clip(np.arange(h) + py, 0, h - 1)
    xx = np.clip(np.arange(w) + px, 0, w - 1)
    return ref[yy][:, xx]


def main():
    ref, oracle = op.load_ref(), op.load_oracle()
    out = {"size": np.array([gg.PU_W, gg.PU_H], np.int32), "ctus": np.array(gg.PU_CTUS, np.int32)}
    cases, counts, counts_frac = [], [], []
    plane_of = {}
    residues = set()
    for k, (bd, qp, R, p, cs) in enumerate(CASES):
        if (bd, p) not in plane_of:
            plane_of[(bd, p)] = len(plane_of)
            out[f"cur{plane_of[(bd, p)]}"], out[f"ref{plane_of[(bd, p)]}"] = planes(bd, p)
        pl = plane_of[(bd, p)]
        cur, refp = out[f"cur{pl}"], out[f"ref{pl}"]
        lam = C.c_double(oracle.fho_lambda_intra(qp, bd))
        rng = np.random.default_rng(4000 + k)
        centres = np.array(CENTRES[cs], np.int16)
        res = np.full((len(gg.PU_CTUS), 593, 5), -1, np.int32)        # mvx, mvy (absolute), SAD, cost, SAD at the centre
        vin = np.zeros((len(gg.PU_CTUS), 593, 2), np.int16)           # the refinement's absolute integer vectors
        frac = np.full((len(gg.PU_CTUS), 593, 5), -1, np.int32)       # satd_int, satd_best, cost_best, mvx, mvy (absolute, quarter units)
        inside = np.zeros((len(gg.PU_CTUS), 593), bool)
        inside_frac = np.zeros((len(gg.PU_CTUS), 593), bool)
        for ci, c in enumerate(gg.PU_CTUS):
            px, py = (int(v) for v in centres[c])
            residues.add(px % 8)          # with R fixed per case, the residue of the window's first column px - R is one to one with it
            shifted = np.ascontiguousarray(displaced(refp, px, py), np.int16)
            where, blocks = gg._pu_blocks(c)
            o, z = np.zeros((len(where), 4), np.int32), np.zeros((len(where), 4), np.int32)
            for r, dst in ((R, o), (0, z)):
                assert ref.href_pattern_search_rect(cur.ctypes.data, shifted.ctypes.data, gg.PU_W, gg.PU_W, gg.PU_H, bd, lam, r, len(where), blocks.reshape(-1),
                                                    dst.reshape(-1)) == len(where)
            assert not z[:, :2].any() and np.abs(o[:, :2]).max() <= R
            res[ci, where, :2] = o[:, :2] + (px, py)
            res[ci, where, 2:4], res[ci, where, 4] = o[:, 2:4], z[:, 2]
            x0, y0, w, h = blocks.T
            for m, flags in ((R, inside), (R + TAPS, inside_frac)):
                # a read at ref' position s is the library's read at s + P only if neither coordinate is clamped: both s and s + P lie inside the picture
                flags[ci, where] = ((x0 + min(px, 0) - m >= 0) & (x0 + w + max(px, 0) + m <= gg.PU_W) &
                                    (y0 + min(py, 0) - m >= 0) & (y0 + h + max(py, 0) + m <= gg.PU_H))
            # the refinement, in ref' coordinates: relative vectors in, relative quarter vectors out
            v = o[:, :2].astype(np.int64)
            pick = np.array(where) % 7 == 0
            v[pick] = rng.integers(-R, R + 1, size=v.shape)[pick]
            b = np.ascontiguousarray(np.concatenate([blocks, v], axis=1), np.int32)
            f = np.zeros((len(where), 7), np.int32)
            assert ref.href_frac_search(cur.ctypes.data, shifted.ctypes.data, gg.PU_W, gg.PU_W, gg.PU_H, bd, lam, len(where), b.reshape(-1), f.reshape(-1)) == len(where)
            vin[ci, where] = v + (px, py)
            frac[ci, where, :3] = f[:, [4, 3, 2]]
            frac[ci, where, 3:] = f[:, :2] + (4 * px, 4 * py)
        valid = res[..., 3] != -1
        four = list(gg.PU_CTUS).index(4)
        assert (inside[four] == valid[four]).all() and (inside_frac[four] == valid[four]).all(), k      # the condition on CTU 4
        assert not (inside & ~valid).any() and not (inside_frac & ~inside).any()
        out[f"centres{k}"], out[f"res{k}"], out[f"in{k}"], out[f"frac{k}"] = centres, res, vin, frac
        out[f"inside{k}"], out[f"inside_frac{k}"] = inside, inside_frac
        cases.append((bd, qp, R, pl))
        counts.append(gg._pu_family_counts(inside))
        counts_frac.append(gg._pu_family_counts(inside_frac))
        print(f"case {k}: bd {bd} qp {qp} R {R} centres {cs}: valid {gg._pu_family_counts(valid)}, inside {counts[-1]}, inside with taps {counts_frac[-1]}, "
              f"moved off the centre {int((np.abs(res[..., :2] - centres[list(gg.PU_CTUS)][:, None, :]).max(axis=-1)[inside] > 0).sum())}, "
              f"fractional winners {int(((frac[..., 3] & 3) | (frac[..., 4] & 3)).astype(bool)[inside_frac].sum())}")
    assert residues == set(range(8)), residues
    out["cases"] = np.array(cases, np.int32)
    out["counts"], out["counts_frac"] = np.array(counts, np.int32), np.array(counts_frac, np.int32)
    gg._pu_save("ref_motion_centred.npz", out)


if __name__ == "__main__":
    main()
