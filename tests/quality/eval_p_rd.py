#!/usr/bin/env python3
"""TEST/QUALITY INFRASTRUCTURE (uses oracle/_ref/libhmref_p.so).  What deciding on RD costs changes: eval_p_intra.py's four columns -- every rule of
eval_p_tree.py with fhevc_p_tree_select's maps, '+merge', '+merge_pu', '+intra' -- and a fifth, '+rd': the maps of fhevc_p_tree_select_rd on the RD records
(fhevc_motion_rd*) of the zero-centred chain's nodes -- SAD search, quarter-sample refinement, re-pricing against neighbour predictors, merge per node, then
the RD stage on the merge records and on the re-priced records with their predictor records --, forced on the reference's own P-picture encode --
reported, never asserted.  The '+rd' column knows 2Nx2N and merge only: it is a statement about two of the seven partition sizes.

eval_p_intra.py's protocol, clips, QPs and rules.  All maps come from the Python restatements (tests/motion_rd_ref.py on the existing ones):
tests/test_gpu_motion_rd.py holds the library on the GPU to the same bits, so no GPU is needed here.  Beside the BD-rate and the share of units whose
full-search depth lies inside the range the report gives how often a depth-0 TU splits, per level and source.

usage: python tests/quality/eval_p_rd.py [--size 832x480] [--frames 4] [--workers 8] [--skip-mask 3] [--json profiles/p_rd_quality.json]
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
import eval_p_intra as base  # noqa: E402
import eval_p_merge_pu as pu  # noqa: E402
import eval_p_tree as et  # noqa: E402
from eval_rd import bd_rate  # noqa: E402
from fasthevc_amd import capi  # noqa: E402

COLUMNS = base.COLUMNS + ("+rd",)
LEVELS = ((0, 1), (1, 5), (5, 21), (21, 85))


def rd_records(oracle, cur, ref, bd, qp, search_range):
    """cur / ref [H, W] samples -> (rd_explicit, rd_merge) [numCtus, 85] MOTION_RD_DTYPE from the restatements of the chain's node stages"""
    import motion_amvp_ref as am
    import motion_merge_ref as mg
    import motion_range_sweep as sw
    import motion_rd_ref as rd
    import motion_refine_ref as mr
    H, W = cur.shape
    R = search_range
    cur, ref = cur.astype(np.int64), ref.astype(np.int64)
    found = sw.PairSweep(oracle, cur, ref, bd, qp, sad=True, rmax=R).records(R)
    cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
    planes = mr.Planes(ref, bd, R + 8)
    nodes = mr.expected(oracle, cur_flat, 0, W, ref, W, H, bd, qp, found["nodes"], R, planes=planes)
    priced, mvp = am.expected(W, H, nodes, nodes, "nodes", qp)
    merge = mg.expected(oracle, cur_flat, 0, W, ref, W, H, bd, qp, priced, R, planes=planes)
    return (rd.expected(cur, ref, W, H, bd, qp, priced, rd.EXPLICIT, R, mvp=mvp, planes=planes), rd.expected(cur, ref, W, H, bd, qp, merge, rd.MERGE, R, planes=planes))


def split_share(rec):
    """per level: the share of the depth-0 TUs of valid nodes that are split"""
    out = []
    for l, (lo, hi) in enumerate(LEVELS):
        v, t = rec["cost_rd"][:, lo:hi] != 0xFFFFFFFF, rec["tu_split"][:, lo:hi]
        tus = 4 if l == 0 else 1
        out.append(sum(int(((t >> b) & 1)[v].sum()) for b in range(tus)) / max(1, int(v.sum()) * tus))
    return out


def _run(job):
    """one clip at one slice QP: the anchor and every rule in the five columns; runs in its own process (HM is single-threaded)"""
    clip, qp, (W, H), nframes, speed, mask = job
    import intra_p_ref as ip
    import motion_merge_ref as mg
    import motion_rd_ref as rd
    import p_tree_ref as tr
    from oracle import oracle_py as op
    eval_p.CLIP, eval_p.SPEED = clip, speed
    lib, oracle = eval_p.load_p(), op.load_oracle()
    ys = eval_p.pan_clip(W, H, nframes)
    tail = lambda seq: (sum(s["bits"] for _, s in seq[2:]), float(np.mean([s["psnr_y"] for _, s in seq[2:]])), sum(s["seconds"] for _, s in seq[2:]))
    anchor = et.encode_forced(lib, ys, qp, None)
    out = {"full_rdo": tail(anchor)}
    frames = range(2, nframes)
    recs = {f: pu.records(oracle, ys[f], ys[f - 1], qp + 6) for f in frames}
    whole = {f: ip.chain_records(oracle, op, ys[f], ys[f - 1], 8, qp + 6, search_range=et.RANGE) for f in frames}
    rds = {f: rd_records(oracle, ys[f], ys[f - 1], 8, qp + 6, et.RANGE) for f in frames}
    out["tu_split_share:explicit"] = np.mean([split_share(rds[f][0]) for f in frames], axis=0).tolist()
    out["tu_split_share:merge"] = np.mean([split_share(rds[f][1]) for f in frames], axis=0).tolist()
    n = ((W + 63) // 64) * ((H + 63) // 64)
    live = np.zeros((n, 16, 16), bool)
    for c in range(n):
        vw, vh = tr.valid_size(c, W, H)
        live[c, :(vh + 3) // 4, :(vw + 3) // 4] = True
    live = live.reshape(n, 256)
    rules = dict({"tree_default": None}, **{name: capi.p_tree_rule(**kw) for name, kw in et.GRID.items()})
    for name, rule in rules.items():
        selects = {"": lambda f: tr.select(recs[f][0][None], W, H, rule=rule), "+merge": lambda f: mg.tree_select(recs[f][0][None], recs[f][1][None], W, H, rule=rule),
                   "+merge_pu": lambda f: mg.tree_select(recs[f][2][None], recs[f][1][None], W, H, rule=rule),
                   "+intra": lambda f: ip.tree_select(whole[f]["shapes"][None], whole[f]["merge"][None], whole[f]["skip"][None], mask, whole[f]["intra"][None], W, H,
                                                      rule=rule),
                   "+rd": lambda f: rd.tree_select(rds[f][0][None], rds[f][1][None], mask, W, H, rule=rule)}
        for suffix in COLUMNS:
            maps = {f: selects[suffix](f) for f in frames}
            seq = et.encode_forced(lib, ys, qp, lambda f, prev: (maps[f][1][0], maps[f][2][0]))
            key = name + suffix
            out[key] = tail(seq)
            out[key + ":agreement"] = [float((seq[f][0] == anchor[f][0]).mean()) for f in frames]
            out[key + ":inside"] = [float(((maps[f][1][0] <= anchor[f][0]) & (anchor[f][0] <= maps[f][2][0]))[live].mean()) for f in frames]
    return (clip, qp), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="832x480")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--speed", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--skip-mask", type=int, default=3, choices=range(4))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "p_rd_quality.json"))
    args = ap.parse_args()
    from multiprocessing import Pool
    W, H = (int(v) for v in args.size.split("x"))
    clips = ("global", "overlaid")
    with Pool(args.workers) as pool:
        res = dict(pool.map(_run, [(clip, qp, (W, H), args.frames, args.speed, args.skip_mask) for clip in clips for qp in et.QPS], chunksize=1))
    names = [n + s for n in ["tree_default"] + list(et.GRID) for s in COLUMNS]
    report = {"tool": "tests/quality/eval_p_rd.py", "protocol": f"{W}x{H}, {args.frames} frames I P P ..., P pictures at QP + 6, POC >= 2 restricted; BD-rate of the "
              "restricted pictures and time in compressSlice against the unrestricted search (eval_p_intra.py's protocol, clips, QPs and rules); its four columns and "
              f"'+rd': fhevc_p_tree_select_rd on the RD records of the zero-centred chain's nodes (2Nx2N and merge only), skip_mask {args.skip_mask}, from the "
              f"restatements at range {et.RANGE}", "qp": list(et.QPS), "grid": et.GRID, "skip_mask": args.skip_mask, "clips": {}}
    for clip in clips:
        ra, pa = [res[(clip, q)]["full_rdo"][0] for q in et.QPS], [res[(clip, q)]["full_rdo"][1] for q in et.QPS]
        ta = sum(res[(clip, q)]["full_rdo"][2] for q in et.QPS)
        entry = {"what": "one global pan of a hetero picture" if clip == "global" else "two transparent motions in opposite directions",
                 "full_rdo": [res[(clip, q)]["full_rdo"] for q in et.QPS],
                 "share_of_depth0_tus_split_per_level": {s: [res[(clip, q)]["tu_split_share:" + s] for q in et.QPS] for s in ("explicit", "merge")}, "variants": {}}
        for name in names:
            pts = [res[(clip, q)][name] for q in et.QPS]
            v = {"points": pts, "bd_rate_percent": bd_rate(ra, pa, [p[0] for p in pts], [p[1] for p in pts]), "compress_slice_time_ratio": ta / sum(p[2] for p in pts),
                 "depth_agreement_with_full_rdo": [float(np.mean(res[(clip, q)][name + ":agreement"])) for q in et.QPS],
                 "full_rdo_depth_inside_the_range": [float(np.mean(res[(clip, q)][name + ":inside"])) for q in et.QPS]}
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
