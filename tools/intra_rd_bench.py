#!/usr/bin/env python3
"""Measurement: the RD estimate of the intra candidate on the device (fhevc_intra_rd_device, the intra instances of k_motion_rd.hip) beside the RD stage on
the same nodes (fhevc_motion_rd_device, whose code this change leaves as it was) and the first pass it follows, on the bench GOP's geometry.
tools/motion_rd_pu_bench.py's protocol.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): pictures 1..63 = 32 130 CTUs per call, the same CTUs the pair stages price.  The
records are real, at range 8: the chain of tools/motion_rd_pu_bench.py up to the folded inter records (part_mode 0, 8, 9) and the merge records' RD
records run once, and so does the first pass of pictures 1..63.  The legs are timed in ONE process, interleaved (every round times each of them once),
each as a window of warmed, repeated launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats
windows with the smallest and largest next to it:
  y      the yardstick: fhevc_motion_rd_device on the re-priced nodes with their predictor records at max_range 8
  plain  the new stage without gate and fold
  fold   the new stage with the calm gate (skip_mask 3) and the fold in place into a copy of the folded inter records (every launch after the first
         finds its own records there; the work per launch is the same, only fewer records change)
  first  fhevc_intra_first_pass_device on the same pictures
Recorded, not asserted: every leg as a ratio to y with the run-to-run spread; per level how often intra wins the fold and how often the gate withholds it;
how the RD tree's depth maps change against the tree on the folded inter records alone.  Before anything is timed the device's records of picture 1 are
compared with the host form.  Quality (BD-rate): not measured.

Needs an MI355X; without one it fails.  Writes profiles/intra_rd.json (--out)."""
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

LEVELS = ((0, 1), (1, 5), (5, 21), (21, 85))
REFERENCE_YARDSTICK_MS = 4.015   # profiles/motion_rd_pu.json: y_rd_explicit_8


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=5, help="launches per window")
    ap.add_argument("--lib", default=None, help="another build of the library to measure (default: the tree's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_rd.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("intra_rd_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("intra_rd_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, R, mask = args.width, args.height, args.frames, args.qp, 8, 3
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
    current = (d8.data_ptr() + W * H, 1, W, W * H, P)   # pictures 1..63: the current picture of every pair
    p = lambda t: t.data_ptr()
    FAM = (85, 124, 384)

    # the inter chain, once: what fhevc_p_tree_rd_frame queues, on the batch
    found, fine, priced = [buf(f) for f in FAM], [buf(f) for f in FAM], [buf(f) for f in FAM]
    mvp = [buf(f, 8) for f in FAM]
    merge, merge_pu, merge_s, shapes, rd_merge, inter = buf(), buf(124), buf(384), buf(), buf(), buf()
    ctx.motion_search_pu_wide_device(*layout, *[p(t) for t in found], stream=st, qp=qp, search_range=R)
    ctx.motion_refine_pu_wide_device(*layout, p(found[0]), p(fine[0]), p(found[1]), p(fine[1]), p(found[2]), p(fine[2]), stream=st, qp=qp, max_range=R)
    ctx.motion_amvp_device(NF, *[p(t) for t in fine], *[p(t) for t in priced], *[p(t) for t in mvp], stream=st, qp=qp)
    ctx.motion_merge_device(*layout, p(priced[0]), p(merge), stream=st, qp=qp, max_range=R)
    ctx.motion_merge_pu_device(*layout, p(priced[0]), p(merge_pu), p(merge_s), stream=st, qp=qp, max_range=R)
    ctx.pu_shape_select_merge_device(*[p(t) for t in priced], p(merge_pu), p(merge_s), P, p(shapes), stream=st)
    ctx.motion_rd_device(*layout, capi.RD_SOURCE_MERGE, p(merge), p(rd_merge), stream=st, qp=qp, max_range=R)
    for mode in (0, 8, 9):
        inputs = ctx.rd_pu_inputs(p(priced[0]), p(priced[1]), p(priced[2]), p(merge_pu), p(merge_s), p(mvp[0]), p(mvp[1]), p(mvp[2]), p(shapes), p(inter) if mode else None)
        ctx.motion_rd_pu_device(*layout, mode, inputs, p(inter), stream=st, qp=qp, max_range=R)
    first = buf()
    ctx.intra_first_pass_device(*current, p(first), stream=st, qp=qp)
    torch.cuda.synchronize()
    del found, fine
    scratch, folded = buf(), buf()
    stage = lambda out, fold=None, m=None, k=0: ctx.intra_rd_device(*current, p(first), p(out), d_fold=fold, d_rd_merge=m, skip_mask=k, stream=st, qp=qp)

    # the result first: picture 1 against the host form, plain and gated + folded
    host = lambda t, dt: t.cpu().numpy().view(dt).reshape(total, 85)
    stage(scratch)
    folded.copy_(inter)
    stage(folded, p(folded), p(rd_merge), mask)
    torch.cuda.synchronize()
    h_first, h_inter, h_merge = host(first, capi.NODE_DTYPE), host(inter, capi.MOTION_RD_PU_DTYPE), host(rd_merge, capi.MOTION_RD_DTYPE)
    h_plain, h_folded = host(scratch, capi.MOTION_RD_PU_DTYPE), host(folded, capi.MOTION_RD_PU_DTYPE)
    cur = pics[1].astype(np.int16)
    equal = (ctx.intra_rd(cur, h_first[:n], origin=0, stride=W, qp=qp).tobytes() == h_plain[:n].tobytes() and
             ctx.intra_rd(cur, h_first[:n], fold=h_inter[:n], rd_merge=h_merge[:n], skip_mask=mask, origin=0, stride=W, qp=qp).tobytes() == h_folded[:n].tobytes())
    print("device equals the host form on picture 1:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture 1 differs from the host form: nothing is timed")

    # what gate and fold chose, and what the tree makes of it
    d_min, d_max = (torch.zeros((total * 256,), dtype=torch.uint8, device="cuda") for _ in range(2))
    maps = []
    for rec in (folded, inter):
        ctx.p_tree_select_rd_pu_device(p(rec), p(rd_merge), mask, P, p(d_min), p(d_max), stream=st)
        torch.cuda.synchronize()
        maps.append((d_min.cpu().numpy().copy(), d_max.cpu().numpy().copy()))
    calm = (h_merge["cost_rd"].astype(np.int64) < h_inter["cost_rd"].astype(np.int64)) & ((h_merge["flags"] & mask) != 0)
    per_level = {}
    for l, (lo, hi) in enumerate(LEVELS):
        v = h_plain["part"][:, lo:hi] != 255
        wins = h_folded["part"][:, lo:hi] == capi.RD_PART_INTRA
        cheaper = v & (h_plain["cost_rd"][:, lo:hi].astype(np.int64) < h_inter["cost_rd"][:, lo:hi].astype(np.int64))
        per_level[str(l)] = {"valid_nodes": int(v.sum()), "share_intra_wins_the_fold": float(wins[v].mean()) if v.any() else 0.0,
                             "share_calm": float(calm[:, lo:hi][v].mean()) if v.any() else 0.0,
                             "share_withheld_by_the_gate_though_cheaper": float((cheaper & calm[:, lo:hi])[v].mean()) if v.any() else 0.0,
                             "share_tu_split": float((h_plain["flags"][:, lo:hi][v] & capi.RD_TU_SPLIT != 0).mean()) if v.any() else 0.0}
    choice = {"per_level": per_level,
              "depth_maps_against_the_tree_on_the_folded_inter_records": {
                  "share_of_depth_min_entries_changed": float((maps[0][0] != maps[1][0]).mean()), "share_of_depth_max_entries_changed": float((maps[0][1] != maps[1][1]).mean()),
                  "mean_depth_max_with_intra": float(maps[0][1].mean()), "mean_depth_max_inter_only": float(maps[1][1].mean())}}
    print("choice:", json.dumps(choice), flush=True)

    runs = {
        "y_rd_explicit_8": lambda: ctx.motion_rd_device(*layout, capi.RD_SOURCE_EXPLICIT, p(priced[0]), p(scratch), d_mvp=p(mvp[0]), stream=st, qp=qp, max_range=R),
        "plain": lambda: stage(scratch),
        "fold": lambda: stage(folded, p(folded), p(rd_merge), mask),
        "first": lambda: ctx.intra_first_pass_device(*current, p(scratch), stream=st, qp=qp),
    }

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    for fn in runs.values():          # warm-up: every shape the timed windows use
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(args.repeats):     # interleaved: one window of each per round
        for name, fn in runs.items():
            ms[name].append(window(fn, args.launches))
    sha = {}
    for name, fn in runs.items():     # one more launch of each, alone, and what it left behind
        fn()
        torch.cuda.synchronize()
        sha[name] = hashlib.sha256((folded if name == "fold" else scratch).cpu().numpy().tobytes()).hexdigest()

    out = {"tool": "tools/intra_rd_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library(args.lib).fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pictures_priced": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8", "max_range": R},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the runs; ms = median of the windows",
           "device_equals_host_form_on_picture_1": bool(equal), "what_gate_and_fold_chose": choice, "quality_bd_rate": "not measured",
           "expectation_from_a_count_of_the_code": "the RD stage's eight transform passes, without the window staging, with line building and two table-driven "
                                                   "predictions (an expectation only; nobody had measured it)",
           "yardstick_in_profiles_motion_rd_pu_json_ms": REFERENCE_YARDSTICK_MS, "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": args.launches, "sha256": sha[name]}
        print(f"{name:18s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  sha256 {sha[name][:16]}", flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios_to_the_yardstick"] = {name: ratio(name, "y_rd_explicit_8") for name in runs if name != "y_rd_explicit_8"}
    out["yardstick_against_profiles_motion_rd_pu_json"] = statistics.median(ms["y_rd_explicit_8"]) / REFERENCE_YARDSTICK_MS
    print("ratios:", json.dumps(out["ratios_to_the_yardstick"]), "yardstick / 4.015 ms:", out["yardstick_against_profiles_motion_rd_pu_json"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
