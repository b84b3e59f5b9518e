#!/usr/bin/env python3
"""TEST/QUALITY INFRASTRUCTURE (uses oracle/_ref/libhmref_p.so).  What the intra candidate (fhevc_intra_p*) changes when the tree takes it
(fhevc_p_tree_select_intra*): eval_p_merge_pu.py's three columns -- every rule of eval_p_tree.py with fhevc_p_tree_select's maps, with the merge variant's
('+merge') and with the merge variant's on merge-aware selection costs ('+merge_pu') -- and a fourth, '+intra': the maps of the tree that takes the intra
candidate on the records of fhevc_p_tree_intra_frame's chain (re-priced refined costs, both merge stages, merge-aware selection, the zero-residual stage
under --skip-mask, the two intra first passes of the current picture, the intra stage), forced on the reference's own P-picture encode -- reported, never
asserted.

eval_p_merge_pu.py's protocol, clips, QPs and rules.  All maps come from the Python restatements (tests/intra_p_ref.py: chain_records and tree_select, built
on the existing restatements and the CPU oracle's first passes): tests/test_gpu_intra_p.py holds the library on the GPU to the same bits, so no GPU is
needed here.  Beside the BD-rate the report gives, per rule, the share of coded nodes whose own cost is the intra cost and the share that is calm.

usage: python tests/quality/eval_p_intra.py [--size 832x480] [--frames 4] [--workers 8] [--skip-mask 3] [--json profiles/p_intra_quality.json]
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
import eval_p_merge_pu as base  # noqa: E402
import eval_p_tree as et  # noqa: E402
from eval_rd import bd_rate  # noqa: E402
from fasthevc_amd import capi  # noqa: E402

COLUMNS = base.COLUMNS + ("+intra",)


def _run(job):
    """one clip at one slice QP: the anchor and every rule in the four columns; runs in its own process (HM is single-threaded)"""
    clip, qp, (W, H), nframes, speed, mask = job
    import intra_p_ref as ip
    import motion_merge_ref as mg
    import motion_skip_ref as sk
    import p_tree_ref as tr
    from oracle import oracle_py as op
    eval_p.CLIP, eval_p.SPEED = clip, speed
    lib, oracle = eval_p.load_p(), op.load_oracle()
    ys = eval_p.pan_clip(W, H, nframes)
    tail = lambda seq: (sum(s["bits"] for _, s in seq[2:]), float(np.mean([s["psnr_y"] for _, s in seq[2:]])), sum(s["seconds"] for _, s in seq[2:]))
    anchor = et.encode_forced(lib, ys, qp, None)
    out = {"full_rdo": tail(anchor)}
    frames = range(2, nframes)
    recs = {f: base.records(oracle, ys[f], ys[f - 1], qp + 6) for f in frames}
    whole = {f: ip.chain_records(oracle, op, ys[f], ys[f - 1], 8, qp + 6, search_range=et.RANGE) for f in frames}
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
                                                      rule=rule)}
        for suffix in COLUMNS:
            maps = {f: selects[suffix](f) for f in frames}
            seq = et.encode_forced(lib, ys, qp, lambda f, prev: (maps[f][1][0], maps[f][2][0]))
            key = name + suffix
            out[key] = tail(seq)
            out[key + ":agreement"] = [float((seq[f][0] == anchor[f][0]).mean()) for f in frames]
            out[key + ":inside"] = [float(((maps[f][1][0] <= anchor[f][0]) & (anchor[f][0] <= maps[f][2][0]))[live].mean()) for f in frames]
            if suffix:
                flags = np.concatenate([maps[f][0]["flags"].reshape(-1) for f in maps])
                coded = (flags & (tr.CROSSING | tr.ABSENT)) == 0
                out[key + ":merge_share"] = float(((flags & mg.MERGED) != 0)[coded].mean())
            if suffix == "+intra":
                taken = np.concatenate([maps[f][0]["pad"][..., 0].reshape(-1) for f in maps]) != 0
                level = np.concatenate([maps[f][0]["level"].reshape(-1) for f in maps])
                calm = np.concatenate([((whole[f]["merge"]["cost_best"] < whole[f]["shapes"]["cost_best"]) & ((whole[f]["skip"]["flags"] & mask) != 0)).reshape(-1)
                                       for f in maps])
                out[key + ":intra_share"] = [float(taken[coded & (level == l)].mean()) if (coded & (level == l)).any() else 0.0 for l in range(4)]
                out[key + ":calm_share"] = [float(calm[coded & (level == l)].mean()) if (coded & (level == l)).any() else 0.0 for l in range(4)]
                out[key + ":skipped_share"] = float(((flags & sk.SKIPPED) != 0)[coded].mean())
    return (clip, qp), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="832x480")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--speed", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--skip-mask", type=int, default=3, choices=range(4))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "p_intra_quality.json"))
    args = ap.parse_args()
    from multiprocessing import Pool
    W, H = (int(v) for v in args.size.split("x"))
    clips = ("global", "overlaid")
    with Pool(args.workers) as pool:
        res = dict(pool.map(_run, [(clip, qp, (W, H), args.frames, args.speed, args.skip_mask) for clip in clips for qp in et.QPS], chunksize=1))
    names = [n + s for n in ["tree_default"] + list(et.GRID) for s in COLUMNS]
    report = {"tool": "tests/quality/eval_p_intra.py", "protocol": f"{W}x{H}, {args.frames} frames I P P ..., P pictures at QP + 6, POC >= 2 restricted; BD-rate of the "
              "restricted pictures and time in compressSlice against the unrestricted search (eval_p_merge_pu.py's protocol, clips, QPs and rules); its three columns and "
              f"'+intra': the tree that takes the intra candidate on the records of fhevc_p_tree_intra_frame's chain, skip_mask {args.skip_mask}, from the restatements "
              f"of the zero-centred chain at range {et.RANGE}", "qp": list(et.QPS), "grid": et.GRID, "skip_mask": args.skip_mask, "clips": {}}
    for clip in clips:
        ra, pa = [res[(clip, q)]["full_rdo"][0] for q in et.QPS], [res[(clip, q)]["full_rdo"][1] for q in et.QPS]
        ta = sum(res[(clip, q)]["full_rdo"][2] for q in et.QPS)
        entry = {"what": "one global pan of a hetero picture" if clip == "global" else "two transparent motions in opposite directions",
                 "full_rdo": [res[(clip, q)]["full_rdo"] for q in et.QPS], "variants": {}}
        for name in names:
            pts = [res[(clip, q)][name] for q in et.QPS]
            v = {"points": pts, "bd_rate_percent": bd_rate(ra, pa, [p[0] for p in pts], [p[1] for p in pts]), "compress_slice_time_ratio": ta / sum(p[2] for p in pts),
                 "depth_agreement_with_full_rdo": [float(np.mean(res[(clip, q)][name + ":agreement"])) for q in et.QPS],
                 "full_rdo_depth_inside_the_range": [float(np.mean(res[(clip, q)][name + ":inside"])) for q in et.QPS]}
            if "+" in name:
                v["share_of_coded_nodes_where_merge_wins"] = [res[(clip, q)][name + ":merge_share"] for q in et.QPS]
            if name.endswith("+intra"):
                v["share_of_coded_nodes_whose_own_cost_is_intra_per_level"] = [res[(clip, q)][name + ":intra_share"] for q in et.QPS]
                v["share_of_coded_nodes_that_are_calm_per_level"] = [res[(clip, q)][name + ":calm_share"] for q in et.QPS]
                v["share_of_coded_nodes_not_descended"] = [res[(clip, q)][name + ":skipped_share"] for q in et.QPS]
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
