#!/usr/bin/env python3
"""Measurement: the merge stage per PU on the device (fhevc_motion_merge_pu_device, k_motion_merge_pu.hip) beside the PU refinement it shares its mapping
with, and the partition-size selection with and without the PUs' merge costs, on the bench GOP's geometry.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 picture pairs = 32 130 CTUs per call.  The records are real: the SAD searches
at range 8 and at range 64 (all three families) and their quarter-sample refinements run once.  Six things are timed in ONE process, interleaved (every
round times each of them once, so a drift of the machine meets all six alike), each as a window of warmed, repeated launches between HIP events on one
explicit stream, ending in a synchronise; every figure is the median of --repeats windows with the smallest and largest next to it:
  a  the stage for all 508 PUs at max_range 8 on the nodes refined at range 8
  b  fhevc_motion_refine_pu_device (both families) at max_range 8 on the PUs found at range 8
  c  the stage at max_range 64 on the nodes refined at range 64
  d  fhevc_motion_refine_pu_wide_device (both PU families) at max_range 64 on the PUs found at range 64
  e  the selection with the merge records (records, costs and bits)
  f  the selection without them (records and costs)
Recorded, not asserted: a / b, c / d, e / f with the run-to-run spread (the smallest and largest ratio of windows of the same round); by candidate count
a / b and c / d would be near 5 / 18 plus the staging, and lists are often shorter than five.  Also recorded (g): per partition size how often a part's
"merged" bit is set, how often `best` changes, and the mean cost_best with and without the merge costs.  Before anything is timed the device's selection
of picture 0 is compared with the host function.  Every leg's figures carry the SHA-256 of the buffers it wrote: the inputs are seeded, so two builds that
behave alike give equal digests.  --lib times another build of the library (A/B of a kernel variant) under the same protocol.

Needs an MI355X; without one it fails.  Writes profiles/motion_merge_pu.json (--out)."""
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
PARTS = {1: "2NxN", 2: "Nx2N", 4: "2NxnU", 5: "2NxnD", 6: "nLx2N", 7: "nRx2N"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=3, help="launches per window of the four motion legs (tens of milliseconds each)")
    ap.add_argument("--select-launches", type=int, default=30, help="launches per window of the two selection legs (tens of microseconds each)")
    ap.add_argument("--lib", default=None, help="another build of the library to measure (default: the tree's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_merge_pu.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("motion_merge_pu_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_merge_pu_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF, lib_path=args.lib)
    n = ctx.num_ctus
    total = P * n
    d8 = torch.from_numpy(np.stack(frames.pan_clip(W, H, NF))).cuda()
    buf = lambda k: torch.zeros((total * k * 16,), dtype=torch.uint8, device="cuda")
    sizes = (85, 124, 384)
    found, refined = [buf(k) for k in sizes], [buf(k) for k in sizes]
    found64, refined64 = [buf(k) for k in sizes], [buf(k) for k in sizes]
    mpu, msmall, mpu64, msmall64, scratch_pu, scratch_small = buf(124), buf(384), buf(124), buf(384), buf(124), buf(384)
    d_shapes, d_shapes_plain = buf(85), buf(85)
    d_costs = torch.zeros((total * 85 * 8,), dtype=torch.int32, device="cuda")
    d_merged = torch.zeros((total * 85,), dtype=torch.int16, device="cuda")
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)
    fp, rp = [t.data_ptr() for t in found], [t.data_ptr() for t in refined]
    fp64, rp64 = [t.data_ptr() for t in found64], [t.data_ptr() for t in refined64]

    ctx.motion_search_pu_wide_device(*layout, fp[0], fp[1], fp[2], stream=st, qp=qp, search_range=8)
    ctx.motion_refine_pu_wide_device(*layout, fp[0], rp[0], fp[1], rp[1], fp[2], rp[2], stream=st, qp=qp, max_range=8)
    ctx.motion_search_pu_wide_device(*layout, fp64[0], fp64[1], fp64[2], stream=st, qp=qp, search_range=64)
    ctx.motion_refine_pu_wide_device(*layout, fp64[0], rp64[0], fp64[1], rp64[1], fp64[2], rp64[2], stream=st, qp=qp, max_range=64)
    ctx.motion_merge_pu_device(*layout, rp[0], mpu.data_ptr(), msmall.data_ptr(), stream=st, qp=qp, max_range=8)
    torch.cuda.synchronize()

    def select(with_merge, shapes):
        if with_merge:
            ctx.pu_shape_select_merge_device(rp[0], rp[1], rp[2], mpu.data_ptr(), msmall.data_ptr(), P, shapes.data_ptr(), d_costs.data_ptr(), d_merged.data_ptr(), stream=st)
        else:
            ctx.pu_shape_select_device(rp[0], rp[1], rp[2], P, shapes.data_ptr(), d_costs.data_ptr(), stream=st)

    runs = {
        "a_merge_pu_8": lambda: ctx.motion_merge_pu_device(*layout, rp[0], scratch_pu.data_ptr(), scratch_small.data_ptr(), stream=st, qp=qp, max_range=8),
        "b_refine_pu_8": lambda: ctx.motion_refine_pu_device(*layout, fp[1], scratch_pu.data_ptr(), fp[2], scratch_small.data_ptr(), stream=st, qp=qp, max_range=8),
        "c_merge_pu_64": lambda: ctx.motion_merge_pu_device(*layout, rp64[0], mpu64.data_ptr(), msmall64.data_ptr(), stream=st, qp=qp, max_range=64),
        "d_refine_pu_64": lambda: ctx.motion_refine_pu_wide_device(*layout, None, None, fp64[1], scratch_pu.data_ptr(), fp64[2], scratch_small.data_ptr(), stream=st, qp=qp,
                                                                   max_range=64),
        "e_select_with_merge": lambda: select(True, d_shapes),
        "f_select_without_merge": lambda: select(False, d_shapes_plain),
    }
    written = {name: [scratch_pu, scratch_small] for name in runs}   # the buffers a leg writes
    written.update(c_merge_pu_64=[mpu64, msmall64], e_select_with_merge=[d_shapes, d_costs, d_merged], f_select_without_merge=[d_shapes_plain, d_costs])

    # the result first: picture 0 against the host function, and what the merge costs change (g)
    host = lambda t, dt, k: t.cpu().numpy().view(dt).reshape(total, k)
    select(False, d_shapes_plain)
    select(True, d_shapes)
    torch.cuda.synchronize()
    plain, merged_rec = host(d_shapes_plain, capi.SHAPE_DTYPE, 85), host(d_shapes, capi.SHAPE_DTYPE, 85)
    bits = d_merged.cpu().numpy().view(np.uint16).reshape(total, 85)
    hrec, hcosts, hbits = capi.pu_shape_select_merge(host(refined[0], capi.MOTION_QPEL_DTYPE, 85)[:n], host(refined[1], capi.MOTION_QPEL_DTYPE, 124)[:n],
                                                     host(refined[2], capi.MOTION_QPEL_DTYPE, 384)[:n], host(mpu, capi.MOTION_MERGE_DTYPE, 124)[:n],
                                                     host(msmall, capi.MOTION_MERGE_DTYPE, 384)[:n], W, H, with_costs=True)
    equal = merged_rec[:n].tobytes() == hrec.tobytes() and bits[:n].tobytes() == hbits.tobytes() and \
        d_costs[:n * 85 * 8].cpu().numpy().view(np.uint32).tobytes() == hcosts.tobytes()
    print("device equals the host function on picture 0:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture 0 differs from the host function: nothing is timed")
    coded = plain["cost_best"] != MARK
    level = np.repeat(np.arange(4), (1, 4, 16, 64))[None, :].repeat(total, 0)
    effect = {"coded_nodes": int(coded.sum()), "share_of_nodes_where_best_changes": float((plain["best"] != merged_rec["best"])[coded].mean()),
              "share_where_best_leaves_2Nx2N": float(((plain["best"] == 0) & (merged_rec["best"] != 0))[coded].mean()),
              "share_of_nodes_with_best_2Nx2N": {"without_merge": float((plain["best"] == 0)[coded].mean()), "with_merge": float((merged_rec["best"] == 0)[coded].mean())},
              "share_where_best_changes_per_level": {str(l): float((plain["best"] != merged_rec["best"])[coded & (level == l)].mean()) for l in range(4)},
              "mean_cost_best": {"without_merge": float(plain["cost_best"][coded].mean()), "with_merge": float(merged_rec["cost_best"][coded].mean())},
              "share_of_parts_with_merged_bit_per_partition_size": {}}
    for p, name in PARTS.items():
        has = coded & (((plain["avail"] | merged_rec["avail"]) >> p) & 1 != 0)
        effect["share_of_parts_with_merged_bit_per_partition_size"][name] = {"part0": float(((bits >> (2 * p)) & 1)[has].mean()), "part1": float(((bits >> (2 * p + 1)) & 1)[has].mean())}
    pm = host(mpu, capi.MOTION_MERGE_DTYPE, 124)
    ok = pm["num"] > 0
    effect["list_lengths_of_the_124"] = {str(k): float((pm["num"][ok] == k).mean()) for k in range(1, 6)}
    print("effect:", json.dumps(effect), flush=True)

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    for fn in runs.values():      # warm-up: every shape the timed windows use
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    launches = {name: args.select_launches if "select" in name else args.launches for name in runs}
    for _ in range(args.repeats):     # interleaved: one window of each per round
        for name, fn in runs.items():
            ms[name].append(window(fn, launches[name]))
    sha = {}
    for name, fn in runs.items():     # one more launch of each, alone, and what it left behind
        fn()
        torch.cuda.synchronize()
        sha[name] = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in written[name])).hexdigest()

    out = {"tool": "tools/motion_merge_pu_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library(args.lib).fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pairs": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8"},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the six runs; ms = median of the windows",
           "device_equals_host_function_on_picture_0": bool(equal), "effect_of_the_merge_costs_at_range_8": effect, "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": launches[name], "sha256": sha[name]}
        print(f"{name:24s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  sha256 {sha[name][:16]}", flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios"] = {"a_over_b": ratio("a_merge_pu_8", "b_refine_pu_8"), "c_over_d": ratio("c_merge_pu_64", "d_refine_pu_64"),
                     "e_over_f": ratio("e_select_with_merge", "f_select_without_merge")}
    out["expectation_by_candidate_count_recorded_not_asserted"] = 5 / 18
    print("ratios:", json.dumps(out["ratios"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
