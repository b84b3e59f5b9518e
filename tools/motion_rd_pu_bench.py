#!/usr/bin/env python3
"""Measurement: the RD stage under a partition size on the device (fhevc_motion_rd_pu_device, the PU instances of k_motion_rd.hip) beside the RD stage on
the same re-priced nodes (fhevc_motion_rd_device, whose code this change leaves as it was), on the bench GOP's geometry.  tools/motion_rd_bench.py's
protocol.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 picture pairs = 32 130 CTUs per call.  The records are real, per range 8 and
64: the SAD searches of all three families, their quarter-sample refinements, the re-pricing with its predictor records, the merge stages of the nodes
and of the PUs and the merge-aware selection run once.  The legs are timed in ONE process, interleaved (every round times each of them once), each as a
window of warmed, repeated launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows
with the smallest and largest next to it.  Per max_range R in {8, 64}:
  y  the yardstick: fhevc_motion_rd_device on the re-priced nodes with their predictor records
  p0 the new stage at part_mode 0            p1 at 1 (2NxN: no tile straddles a cut above the 8x8 nodes)
  p4 at 4 (2NxnU: the tiles of the 16x16 nodes straddle, the 8x8 nodes have no such size)
  p8 at 8 (the selection's best)              p9f at 9 folded in place into a copy of p8's records
  seq the three launches 0, 8 folded, 9 folded on one stream
Recorded, not asserted: every leg as a ratio to y with the run-to-run spread; per level how often the folded winner is not 2Nx2N and how often it is the
selection's best; how the RD tree's depth maps change against fhevc_p_tree_select_rd_device on the 2Nx2N records alone.  Before anything is timed the
device's records of picture pair 0 are compared with the host form.

Needs an MI355X; without one it fails.  Writes profiles/motion_rd_pu.json (--out)."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fasthevc_amd import capi, frames  # noqa: E402

MARK = 0xFFFFFFFF
LEVELS = ((0, 1), (1, 5), (5, 21), (21, 85))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=5, help="launches (seq: sequences) per window")
    ap.add_argument("--lib", default=None, help="another build of the library to measure (default: the tree's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_rd_pu.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("motion_rd_pu_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_rd_pu_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF, lib_path=args.lib)
    n = ctx.num_ctus
    total = P * n
    pics = frames.pan_clip(W, H, NF)
    d8 = torch.from_numpy(np.stack(pics)).cuda()
    buf = lambda per=85, nbytes=16: torch.zeros((total * per * nbytes,), dtype=torch.uint8, device="cuda")
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)
    p = lambda t: t.data_ptr()
    FAM = (85, 124, 384)

    chain = {}
    for R in (8, 64):
        found, fine, priced = [buf(f) for f in FAM], [buf(f) for f in FAM], [buf(f) for f in FAM]
        mvp = [buf(f, 8) for f in FAM]
        merge, merge_pu, merge_s, shapes, rd_merge = buf(), buf(124), buf(384), buf(), buf()
        ctx.motion_search_pu_wide_device(*layout, *[p(t) for t in found], stream=st, qp=qp, search_range=R)
        ctx.motion_refine_pu_wide_device(*layout, p(found[0]), p(fine[0]), p(found[1]), p(fine[1]), p(found[2]), p(fine[2]), stream=st, qp=qp, max_range=R)
        ctx.motion_amvp_device(NF, *[p(t) for t in fine], *[p(t) for t in priced], *[p(t) for t in mvp], stream=st, qp=qp)
        ctx.motion_merge_device(*layout, p(priced[0]), p(merge), stream=st, qp=qp, max_range=R)
        ctx.motion_merge_pu_device(*layout, p(priced[0]), p(merge_pu), p(merge_s), stream=st, qp=qp, max_range=R)
        ctx.pu_shape_select_merge_device(*[p(t) for t in priced], p(merge_pu), p(merge_s), P, p(shapes), stream=st)
        ctx.motion_rd_device(*layout, capi.RD_SOURCE_MERGE, p(merge), p(rd_merge), stream=st, qp=qp, max_range=R)
        torch.cuda.synchronize()
        del found, fine
        chain[R] = dict(priced=priced, mvp=mvp, merge=merge, merge_pu=merge_pu, merge_s=merge_s, shapes=shapes, rd_merge=rd_merge,
                        inputs=lambda fold=None, q=priced, m=(merge_pu, merge_s), v=mvp, s=shapes: ctx.rd_pu_inputs(p(q[0]), p(q[1]), p(q[2]), p(m[0]), p(m[1]), p(v[0]), p(v[1]),
                                                                                                                  p(v[2]), p(s), fold))
    scratch, folded, best = buf(), buf(), buf()
    pu_launch = lambda R, mode, out, fold=None: ctx.motion_rd_pu_device(*layout, mode, chain[R]["inputs"](fold), p(out), stream=st, qp=qp, max_range=R)

    def sequence(R, out):
        pu_launch(R, 0, out)
        pu_launch(R, 8, out, p(out))
        pu_launch(R, 9, out, p(out))

    # the result first: picture pair 0 of the folded sequence at range 8 against the host form, launch by launch
    sequence(8, folded)
    torch.cuda.synchronize()
    host = lambda t, dt, per=85: t.cpu().numpy().view(dt).reshape(total, per)
    c8 = chain[8]
    arrays = [host(t, capi.MOTION_QPEL_DTYPE, f)[:n] for t, f in zip(c8["priced"], FAM)] + [host(c8["merge_pu"], capi.MOTION_MERGE_DTYPE, 124)[:n],
              host(c8["merge_s"], capi.MOTION_MERGE_DTYPE, 384)[:n]] + [host(t, capi.MOTION_MVP_DTYPE, f)[:n] for t, f in zip(c8["mvp"], FAM)] + [
              host(c8["shapes"], capi.SHAPE_DTYPE)[:n]]
    cur, ref = pics[1].astype(np.int16), pics[0].astype(np.int16)
    h = ctx.motion_rd_pu(cur, ref, 0, *arrays, origin=0, stride=W, qp=qp, max_range=8)
    for mode in (8, 9):
        h = ctx.motion_rd_pu(cur, ref, mode, *arrays, fold=h, origin=0, stride=W, qp=qp, max_range=8)
    folded_h = host(folded, capi.MOTION_RD_PU_DTYPE)
    equal = h.tobytes() == folded_h[:n].tobytes()
    print("device equals the host form on picture pair 0:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture pair 0 differs from the host form: nothing is timed")

    # what the fold chose, and what the tree makes of it
    choice = {}
    d_min, d_max = (torch.zeros((total * 256,), dtype=torch.uint8, device="cuda") for _ in range(2))
    for R in (8, 64):
        sequence(R, folded)
        pu_launch(R, 0, scratch)
        maps = []
        for rec in (folded, scratch):
            ctx.p_tree_select_rd_pu_device(p(rec), p(chain[R]["rd_merge"]), 3, P, p(d_min), p(d_max), stream=st)
            torch.cuda.synchronize()
            maps.append((d_min.cpu().numpy().copy(), d_max.cpu().numpy().copy()))
        f, s = host(folded, capi.MOTION_RD_PU_DTYPE), host(chain[R]["shapes"], capi.SHAPE_DTYPE)
        per_level = {}
        for l, (lo, hi) in enumerate(LEVELS):
            v = f["part"][:, lo:hi] != 255
            per_level[str(l)] = {"valid_nodes": int(v.sum()), "share_winner_not_2Nx2N": float((f["part"][:, lo:hi][v] != 0).mean()) if v.any() else 0.0,
                                 "share_winner_is_the_selections_best": float((f["part"][:, lo:hi][v] == s["best"][:, lo:hi][v]).mean()) if v.any() else 0.0,
                                 "share_winner_with_a_merged_part": float((f["merged"][:, lo:hi][v] != 0).mean()) if v.any() else 0.0}
        choice[str(R)] = {"per_level": per_level,
                          "depth_maps_against_the_tree_on_2Nx2N_records": {
                              "share_of_depth_min_entries_changed": float((maps[0][0] != maps[1][0]).mean()), "share_of_depth_max_entries_changed": float((maps[0][1] != maps[1][1]).mean()),
                              "mean_depth_max_folded": float(maps[0][1].mean()), "mean_depth_max_2Nx2N": float(maps[1][1].mean())}}
    print("choice:", json.dumps(choice), flush=True)

    runs = {}
    for R in (8, 64):
        c = chain[R]
        runs[f"y_rd_explicit_{R}"] = lambda R=R, c=c: ctx.motion_rd_device(*layout, capi.RD_SOURCE_EXPLICIT, p(c["priced"][0]), p(scratch), d_mvp=p(c["mvp"][0]), stream=st, qp=qp,
                                                                          max_range=R)
        for mode in (0, 1, 4, 8):
            runs[f"p{mode}_{R}"] = lambda R=R, mode=mode: pu_launch(R, mode, scratch)
        runs[f"p9f_{R}"] = lambda R=R: pu_launch(R, 9, scratch, p(best))       # into a second buffer: `best` stays what part_mode 8 wrote, so every launch folds alike
        runs[f"seq_{R}"] = lambda R=R: sequence(R, folded)
    prepare = {f"p9f_{R}": (lambda R=R: pu_launch(R, 8, best)) for R in (8, 64)}

    def window(name, fn, launches):
        if name in prepare:
            prepare[name]()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    for name, fn in runs.items():      # warm-up: every shape the timed windows use
        if name in prepare:
            prepare[name]()
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(args.repeats):     # interleaved: one window of each per round
        for name, fn in runs.items():
            ms[name].append(window(name, fn, args.launches))
    sha = {}
    for name, fn in runs.items():     # one more launch of each, alone, and what it left behind
        if name in prepare:
            prepare[name]()
        fn()
        torch.cuda.synchronize()
        sha[name] = hashlib.sha256((folded if name.startswith("seq") else scratch).cpu().numpy().tobytes()).hexdigest()

    out = {"tool": "tools/motion_rd_pu_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library(args.lib).fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pairs": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8"},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the runs; ms = median of the windows; seq: ms per "
                     "sequence of three launches",
           "device_equals_host_form_on_picture_pair_0": bool(equal), "what_the_fold_chose": choice, "quality_bd_rate": "not measured",
           "expectation_from_a_count_of_the_code": "one more prediction on at most two of the four waves plus a few record loads per lane (an expectation only)",
           "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": args.launches, "sha256": sha[name]}
        print(f"{name:18s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  sha256 {sha[name][:16]}", flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios_to_the_yardstick"] = {name: ratio(name, f"y_rd_explicit_{name.rsplit('_', 1)[1]}") for name in runs if not name.startswith("y_")}
    print("ratios:", json.dumps(out["ratios_to_the_yardstick"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
