"""tests/golden/ref_motion_candidates.npz: what the REFERENCE's own list functions return -- TComDataCU::fillMvpCand (TComDataCU.cpp:2578-2716) and
TComDataCU::getInterMergeCandidates (:2142-2484) -- through href_mc_set_field / href_mc_query of oracle/ref_rdo_harness.cpp, on motion fields set by hand;
and the reference's TComRdCost::getCost(b), b = 0..66, at every QP, with getBitsOfVectorWithPredictor on the differences of motion_candidates_cases.DIFFS
(href_mv_bit_tables).  The file pins what the three candidate stages (fhevc_motion_amvp*, fhevc_motion_merge*, fhevc_motion_merge_pu*) rest on: the five
positions of every node, PU and small PU, the same-level node behind each, the coding-order rule, AMVP's own-CU rule, the merge stage's second-PU
exclusions, both list rules and the bit table (tests/test_motion_candidates_pin.py without a GPU, tests/test_gpu_motion_candidates_pin.py for the kernels).

Stored per draw, explicitly: the vectors and marker flags of 9 x 85 nodes, 9 x 124 PUs and 9 x 384 small PUs of the 168 x 152 picture, and the
reference's answer (motion_candidates_cases.REC int16) for every INSIDE entry.  Two kinds of draw alternate: AMVP draws take vectors from
motion_amvp_ref.POOL (int16 extremes included; one PU in twenty holds +-2^k components instead, so that chosen differences of 39 bits and more are
many) and record the AMVP list; merge draws take vectors from a pool within the reach of max_range 8 and record both lists.  Three records in ten are
markers; the 64x64 nodes of CTUs 0, 3 and 4 never are and that of CTU 1 is in every second pair of draws, because on the four INSIDE 64x64 nodes AL can
supply the list only while the node above is a marker and AR only while it is none; the 64x64 nodes of CTUs 0, 1 and 3 hold three different vectors of
the pool, so that the AMVP prune does not take the one candidate the schedule is for.  Eight draws is the smallest number at which both are seen four times.

CPU only; needs oracle/_ref (python __graft_entry__.py builds it where the reference's sources are).  Integers only; the archive is written with fixed
time stamps, so a second run gives the same bytes:

    python tests/quality/gen_motion_candidates_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import motion_amvp_ref as ar  # noqa: E402
import motion_candidates_cases as cc  # noqa: E402
import oracle_py as op  # noqa: E402
from gen_quant_golden import write_archive  # noqa: E402


def make_draw(d, kind):
    """-> (mv {family: [N, per, 2] int16}, marker {family: [N, per] uint8})"""
    rng = np.random.default_rng(4200 + d)
    pool = np.array(ar.POOL if kind == "amvp" else cc.MERGE_POOL, np.int16)
    mv, marker = {}, {}
    for f in cc.FAMILIES:
        shape = (cc.N, cc.PER[f])
        mv[f] = pool[rng.integers(0, len(pool), size=shape)]
        marker[f] = (rng.random(shape) < cc.MARKER_RATE).astype(np.uint8)
        if kind == "amvp" and f != "nodes":
            far = rng.random(shape) < 0.05
            comp = (rng.choice([-1, 1], size=shape + (2,)) * (1 << rng.integers(8, 15, size=shape + (2,)))).astype(np.int16)
            mv[f] = np.where(far[..., None], comp, mv[f])
    marker["nodes"][[0, 3, 4], 0] = 0
    marker["nodes"][1, 0] = (d >> 1) & 1
    for i, c in enumerate((0, 1, 3)):          # three different vectors, so that the AMVP prune does not take the one candidate the schedule is for
        mv["nodes"][c, 0] = pool[(d + i) % len(pool)]
    return mv, marker


def main():
    lib = op.bind_candidates(op.load_ref())
    out = {"kind": np.array([k == "merge" for k in cc.KINDS], np.uint8)}
    draws = []
    for d, kind in enumerate(cc.KINDS):
        mv, marker = make_draw(d, kind)
        draws.append((mv, marker, cc.record(lib, mv, marker, kind == "merge")))
    for f in cc.FAMILIES:
        out[f"mv_{f}"] = np.stack([d[0][f] for d in draws])
        out[f"marker_{f}"] = np.stack([d[1][f] for d in draws])
        out[f"ref_{f}"] = np.stack([d[2][f] for d in draws])
    out["cost"], out["bit_counts"] = cc.tables_from(lib)
    out["bit_pairs"] = cc.bit_pairs()
    seen = cc.coverage(out)
    for key in sorted(seen, key=str):
        print(key, seen[key])
    for f in cc.FAMILIES:
        n = int(cc.compared(f, out[f"marker_{f}"]).sum())
        m = int(cc.compared(f, out[f"marker_{f}"])[list(cc.MERGE_DRAWS)].sum())
        print(f"{f}: {n} compared entries, {m} of them in merge draws, {int(cc.tables(f)[2].sum()) * len(cc.MERGE_DRAWS)} INSIDE entries in merge draws")
        for lvl in ar.LEVELS[f]:
            for name in cc.NAMES:
                key = ("amvp", f, lvl, name)
                assert (seen[key] == 0) if key in cc.EXCUSED else (seen[key] >= cc.required(f, lvl)), (key, seen[key])
    write_archive(cc.GOLDEN, out)
    print(cc.GOLDEN, os.path.getsize(cc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
