#!/usr/bin/env python3
"""TEST/QUALITY INFRASTRUCTURE (uses oracle/_ref/libhmref_p.so).  What the PUs' merge costs (fhevc_motion_merge_pu*) change when the partition-size selection
takes them (fhevc_pu_shape_select_merge*): eval_p_merge.py's two columns -- every rule of eval_p_tree.py with fhevc_p_tree_select's maps and with the merge
variant's maps -- and a third, the merge variant's tree on MERGE-AWARE selection costs ('+merge_pu': what fhevc_p_tree_merge_pu_frame computes), forced on
the reference's own P-picture encode -- reported, never asserted.

eval_p_merge.py's protocol, clips, QPs and rules.  All maps come from the Python restatements of the chain (zero-centred SAD search at range 8,
quarter-sample refinement, both merge stages, partition-size selection, tree): tests/test_gpu_motion_merge_pu.py holds the library on the GPU to the same
bits, so no GPU is needed here.

usage: python tests/quality/eval_p_merge_pu.py [--size 832x480] [--frames 4] [--workers 8] [--json profiles/p_merge_pu_quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))       # tests/: the restatements
import eval_p  # noqa: E402
import eval_p_tree as et  # noqa: E402
from eval_rd import bd_rate  # noqa: E402
from fasthevc_amd import capi  # noqa: E402

COLUMNS = ("", "+merge", "+merge_pu")


def records(oracle, cur, ref, qp):
    """(the selection's records, the merge records of the nodes, the selection's records on merge-aware costs, its merged bits) [numCtus, 85] of one pair
    through the restatements"""
    import motion_merge_pu_ref as mpr
    import motion_merge_ref as mg
    import motion_range_sweep as sw
    import motion_refine_pu_ref as rp
    import motion_refine_ref as mr
    import pu_shape_ref as sr
    H, W = cur.shape
    cur, ref = cur.astype(np.int64), ref.astype(np.int64)
    found = sw.PairSweep(oracle, cur, ref, 8, qp, sad=True, rmax=et.RANGE).records(et.RANGE)
    cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
    planes = mr.Planes(ref, 8, et.RANGE + 8)
    nodes = mr.expected(oracle, cur_flat, 0, W, ref, W, H, 8, qp, found["nodes"], et.RANGE, planes=planes)
    pu = rp.expected(oracle, cur, ref, 8, qp, found["pu"], et.RANGE, "pu", planes=planes)
    small = rp.expected(oracle, cur, ref, 8, qp, found["small"], et.RANGE, "small", planes=planes)
    merge = mg.expected(oracle, cur_flat, 0, W, ref, W, H, 8, qp, nodes, et.RANGE, planes=planes)
    mpu, msmall = (mpr.expected(oracle, cur_flat, 0, W, ref, W, H, 8, qp, nodes, et.RANGE, f, planes=planes) for f in ("pu", "small"))
    aware, _, bits = mpr.select(nodes[None], pu[None], small[None], mpu[None], msmall[None], W, H)
    return sr.select(nodes[None], pu[None], small[None], W, H)[0][0], merge, aware[0], bits[0]


def _run(job):
    """one clip at one slice QP: the anchor and every rule in the three columns; runs in its own process (HM is single-threaded)"""
    clip, qp, (W, H), nframes, speed = job
    import motion_merge_ref as mg
    import p_tree_ref as tr
    from oracle import oracle_py as op
    eval_p.CLIP, eval_p.SPEED = clip, speed
    lib, oracle = eval_p.load_p(), op.load_oracle()
    ys = eval_p.pan_clip(W, H, nframes)
    tail = lambda seq: (sum(s["bits"] for _, s in seq[2:]), float(np.mean([s["psnr_y"] for _, s in seq[2:]])), sum(s["seconds"] for _, s in seq[2:]))
    anchor = et.encode_forced(lib, ys, qp, None)
    out = {"full_rdo": tail(anchor)}
    recs = {f: records(oracle, ys[f], ys[f - 1], qp + 6) for f in range(2, nframes)}
    n = ((W + 63) // 64) * ((H + 63) // 64)
    live = np.zeros((n, 16, 16), bool)
    for c in range(n):
        vw, vh = tr.valid_size(c, W, H)
        live[c, :(vh + 3) // 4, :(vw + 3) // 4] = True
    live = live.reshape(n, 256)
    plain_best = np.concatenate([recs[f][0]["best"].reshape(-1) for f in recs])
    aware_best = np.concatenate([recs[f][2]["best"].reshape(-1) for f in recs])
    coded_sel = plain_best != 255
    out["selection"] = {"share_of_nodes_where_best_changes": float((plain_best != aware_best)[coded_sel].mean()),
                        "share_of_nodes_with_a_merged_bit": float((np.concatenate([recs[f][3].reshape(-1) for f in recs]) != 0)[coded_sel].mean())}
    rules = dict({"tree_default": None}, **{name: capi.p_tree_rule(**kw) for name, kw in et.GRID.items()})
    for name, rule in rules.items():
        selects = {"": lambda r: tr.select(r[0][None], W, H, rule=rule), "+merge": lambda r: mg.tree_select(r[0][None], r[1][None], W, H, rule=rule),
                   "+merge_pu": lambda r: mg.tree_select(r[2][None], r[1][None], W, H, rule=rule)}
        for suffix in COLUMNS:
            maps = {f: selects[suffix](recs[f]) for f in recs}
            seq = et.encode_forced(lib, ys, qp, lambda f, prev: (maps[f][1][0], maps[f][2][0]))
            key = name + suffix
            out[key] = tail(seq)
            out[key + ":agreement"] = [float((seq[f][0] == anchor[f][0]).mean()) for f in range(2, nframes)]
            out[key + ":inside"] = [float(((maps[f][1][0] <= anchor[f][0]) & (anchor[f][0] <= maps[f][2][0]))[live].mean()) for f in range(2, nframes)]
            if suffix:
                flags = np.concatenate([maps[f][0]["flags"].reshape(-1) for f in maps])
                coded = (flags & (tr.CROSSING | tr.ABSENT)) == 0
                out[key + ":merge_share"] = float(((flags & mg.MERGED) != 0)[coded].mean())
    return (clip, qp), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="832x480")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--speed", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "p_merge_pu_quality.json"))
    args = ap.parse_args()
    from multiprocessing import Pool
    W, H = (int(v) for v in args.size.split("x"))
    clips = ("global", "overlaid")
    with Pool(args.workers) as pool:
        res = dict(pool.map(_run, [(clip, qp, (W, H), args.frames, args.speed) for clip in clips for qp in et.QPS], chunksize=1))
    names = [n + s for n in ["tree_default"] + list(et.GRID) for s in COLUMNS]
    report = {"tool": "tests/quality/eval_p_merge_pu.py", "protocol": f"{W}x{H}, {args.frames} frames I P P ..., P pictures at QP + 6, POC >= 2 restricted; BD-rate of the "
              "restricted pictures and time in compressSlice against the unrestricted search (eval_p_merge.py's protocol, clips, QPs and rules); every rule with "
              "fhevc_p_tree_select's maps, with the merge variant's ('+merge') and with the merge variant's on merge-aware selection costs ('+merge_pu'), from the "
              f"restatements of the zero-centred chain at range {et.RANGE}", "qp": list(et.QPS), "grid": et.GRID, "clips": {}}
    for clip in clips:
        ra, pa = [res[(clip, q)]["full_rdo"][0] for q in et.QPS], [res[(clip, q)]["full_rdo"][1] for q in et.QPS]
        ta = sum(res[(clip, q)]["full_rdo"][2] for q in et.QPS)
        entry = {"what": "one global pan of a hetero picture" if clip == "global" else "two transparent motions in opposite directions",
                 "full_rdo": [res[(clip, q)]["full_rdo"] for q in et.QPS], "selection": [res[(clip, q)]["selection"] for q in et.QPS], "variants": {}}
        for name in names:
            pts = [res[(clip, q)][name] for q in et.QPS]
            v = {"points": pts, "bd_rate_percent": bd_rate(ra, pa, [p[0] for p in pts], [p[1] for p in pts]), "compress_slice_time_ratio": ta / sum(p[2] for p in pts),
                 "depth_agreement_with_full_rdo": [float(np.mean(res[(clip, q)][name + ":agreement"])) for q in et.QPS],
                 "full_rdo_depth_inside_the_range": [float(np.mean(res[(clip, q)][name + ":inside"])) for q in et.QPS]}
            if "+merge" in name:
                v["share_of_coded_nodes_where_merge_wins"] = [res[(clip, q)][name + ":merge_share"] for q in et.QPS]
            entry["variants"][name] = v
            print(f"{clip:9s} {name:38s} BD-rate {v['bd_rate_percent']:+7.2f} %   compressSlice {v['compress_slice_time_ratio']:5.2f}x faster   inside "
                  f"{np.mean(v['full_rdo_depth_inside_the_range']):.3f}", flush=True)
        report["clips"][clip] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.json)


if __name__ == "__main__":
    main()
