"""tests/golden/ref_pattern_search_pu_wide.npz: what the REFERENCE's own TEncSearch::xPatternSearch (SAD, w x h patterns) returns at HM's own
SearchRange for the 85 nodes, the 124 PUs and the 384 small PUs of five CTUs of the ragged 176 x 144 picture -- the file
fhevc_motion_search_pu_wide is pinned to (tests/test_oracle_golden_motion_pu_wide.py without a GPU, tests/test_gpu_motion_pu_wide.py on one).
The layout is tests/golden/ref_pattern_search_pu.npz's (tests/motion_golden.py: SearchCase); picture, CTUs, entries and the call into the
reference are oracle/gen_golden.py's (_pu_planes, _pu_blocks, _pu_search_case), used as they are.  At R = 64 every window on this picture
reaches the replicated border: that is the point of the file.

CPU only; needs oracle/_ref (python __graft_entry__.py builds it where the reference's sources are).  Planes and integers only:

    python tests/quality/gen_motion_pu_wide_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_golden as gg  # noqa: E402
import oracle_py as op  # noqa: E402
from fasthevc_amd import frames  # noqa: E402

# pan clips whose two overlaid motions both exceed 8 samples per picture: (seed, v_structure, v_noise)
WIDE_PANS = {"panA": (170, 19, -13), "panB": (171, -27, 35)}
# (bit depth, QP, range, content): 8 bit at HM's range and at an odd one on both pans; 10 and 12 bit with the low bits populated; the two contents
# whose ties raster order decides over 16 641 vectors ("white", "checker": gen_golden._pu_planes)
WIDE_CASES = ((8, 32, 64, "panA"), (8, 22, 33, "panB"), (8, 37, 64, "panB"), (8, 45, 33, "panA"), (10, 27, 64, "panA"), (12, 32, 24, "panB"),
              (8, 32, 64, "white"), (10, 32, 64, "checker"))


def planes(bd, content):
    """-> (cur, ref) int16 [H, W]"""
    if content not in WIDE_PANS:
        return gg._pu_planes(bd, content)
    seed, vs, vn = WIDE_PANS[content]
    ys = frames.pan_clip(gg.PU_W, gg.PU_H, 2, seed=seed, v_structure=vs, v_noise=vn)
    ref, cur = (y.astype(np.int64) << (bd - 8) for y in ys)
    if bd > 8:  # use the low bits too
        cur = cur + np.random.default_rng(bd).integers(0, 1 << (bd - 8), size=cur.shape)
        ref = ref + np.random.default_rng(bd + 1).integers(0, 1 << (bd - 8), size=ref.shape)
    return np.ascontiguousarray(cur, np.int16), np.ascontiguousarray(ref, np.int16)


def main():
    ref, oracle = op.load_ref(), op.load_oracle()
    pics, plane_of = [], {}
    out = {"size": np.array([gg.PU_W, gg.PU_H], np.int32), "ctus": np.array(gg.PU_CTUS, np.int32)}
    cases, counts = [], np.zeros(3, np.int64)
    for k, (bd, qp, R, content) in enumerate(WIDE_CASES):
        if (bd, content) not in plane_of:
            plane_of[(bd, content)] = len(pics)
            pics.append(planes(bd, content))
        p = plane_of[(bd, content)]
        res = gg._pu_search_case(ref, oracle, *pics[p], bd, qp, R)
        valid = res[..., 3] != -1
        per_case = gg._pu_family_counts(valid)
        counts += per_case
        longest = [int(np.abs(res[..., s, :2][valid[..., s]]).max()) for s in (slice(0, 85), slice(85, 209), slice(209, 593))]
        print(f"case {k}: bd {bd} qp {qp} R {R} {content}: valid {per_case}, longest |mv| component per family {longest}")
        if content in WIDE_PANS:   # the golden vectors are long in every family
            assert min(longest) > 8, (k, longest)
        out[f"res{k}"] = res
        cases.append((bd, qp, R, p))
    for p, (cur, refp) in enumerate(pics):
        out[f"cur{p}"], out[f"ref{p}"] = cur, refp
    out["cases"], out["counts"] = np.array(cases, np.int32), counts.astype(np.int32)
    print("valid entries (nodes, PUs, small PUs):", counts.tolist(), "in", len(cases), "cases")
    gg._pu_save("ref_pattern_search_pu_wide.npz", out)


if __name__ == "__main__":
    main()
