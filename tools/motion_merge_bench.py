#!/usr/bin/env python3
"""Measurement: the merge stage on the device (fhevc_motion_merge_device, k_motion_merge.hip) beside the square refinement it shares its mapping with, and
the tree decision with and without the merge costs, on the bench GOP's geometry.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 picture pairs = 32 130 CTUs per call.  The records are real: the SAD searches
at range 8 (all three families) and at range 64 (the nodes), their quarter-sample refinements and the partition-size selection run once.  Six things are
timed in ONE process, interleaved (every round times each of them once, so a drift of the machine meets all six alike), each as a window of warmed,
repeated launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows with the smallest
and largest next to it (5 launches per window for the legs of milliseconds, 50 for the two tree legs of tens of microseconds):
  a  the merge stage at max_range 8 on the nodes refined at range 8
  b  fhevc_motion_refine_device at max_range 8 on the nodes those came from
  c  the merge stage at max_range 64 on the nodes refined at range 64
  d  fhevc_motion_refine_device at max_range 64 on the nodes those came from
  e  the tree decision with the merge costs (maps and records)
  f  the tree decision without them
Recorded, not asserted: a / b, c / d, e / f with the run-to-run spread (the smallest and largest ratio of windows of the same round); by candidate count
a / b and c / d would be near 5 / 18 plus the staging.  Also recorded: the share of coded nodes whose merge cost is the smaller one, and the mean own cost
with and without it.  Before anything is timed the device's merge-tree records of picture 0 are compared with the host function.

Needs an MI355X; without one it fails.  Writes profiles/motion_merge.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fasthevc_amd import capi, frames  # noqa: E402

REC_BYTES = 85 * 16
MARK = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=5, help="launches per window of the four motion legs (milliseconds each)")
    ap.add_argument("--tree-launches", type=int, default=50, help="launches per window of the two tree legs (tens of microseconds each), as tools/p_tree_bench.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_merge.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("motion_merge_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_merge_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    total = P * n
    d8 = torch.from_numpy(np.stack(frames.pan_clip(W, H, NF))).cuda()
    buf = lambda k: torch.zeros((total * k * 16,), dtype=torch.uint8, device="cuda")
    found = [buf(k) for k in (85, 124, 384)]
    refined = [buf(k) for k in (85, 124, 384)]
    found64, refined64 = buf(85), buf(85)
    merge8, merge64, scratch, d_shapes, d_tree = buf(85), buf(85), buf(85), buf(85), buf(85)
    d_min = torch.zeros((total * 256,), dtype=torch.uint8, device="cuda")
    d_max = torch.zeros_like(d_min)
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)
    fp = [t.data_ptr() for t in found]
    rp = [t.data_ptr() for t in refined]

    ctx.motion_search_pu_wide_device(*layout, fp[0], fp[1], fp[2], stream=st, qp=qp, search_range=8)
    ctx.motion_refine_pu_wide_device(*layout, fp[0], rp[0], fp[1], rp[1], fp[2], rp[2], stream=st, qp=qp, max_range=8)
    ctx.pu_shape_select_device(rp[0], rp[1], rp[2], P, d_shapes.data_ptr(), None, stream=st)
    ctx.motion_search_pu_wide_device(*layout, found64.data_ptr(), None, None, stream=st, qp=qp, search_range=64)
    ctx.motion_refine_device(*layout, found64.data_ptr(), refined64.data_ptr(), stream=st, qp=qp, max_range=64)
    ctx.motion_merge_device(*layout, rp[0], merge8.data_ptr(), stream=st, qp=qp, max_range=8)
    torch.cuda.synchronize()

    def tree(with_merge):
        if with_merge:
            ctx.p_tree_select_merge_device(d_shapes.data_ptr(), merge8.data_ptr(), P, d_min.data_ptr(), d_max.data_ptr(), d_tree.data_ptr(), stream=st)
        else:
            ctx.p_tree_select_device(d_shapes.data_ptr(), P, d_min.data_ptr(), d_max.data_ptr(), d_tree.data_ptr(), stream=st)

    runs = {
        "a_merge_8": lambda: ctx.motion_merge_device(*layout, rp[0], scratch.data_ptr(), stream=st, qp=qp, max_range=8),
        "b_refine_8": lambda: ctx.motion_refine_device(*layout, fp[0], scratch.data_ptr(), stream=st, qp=qp, max_range=8),
        "c_merge_64": lambda: ctx.motion_merge_device(*layout, refined64.data_ptr(), merge64.data_ptr(), stream=st, qp=qp, max_range=64),
        "d_refine_64": lambda: ctx.motion_refine_device(*layout, found64.data_ptr(), scratch.data_ptr(), stream=st, qp=qp, max_range=64),
        "e_tree_with_merge": lambda: tree(True),
        "f_tree_without_merge": lambda: tree(False),
    }

    # the result first: picture 0 against the host function, and what the merge stage changes
    host = lambda t, dt: t.cpu().numpy().view(dt).reshape(total, 85)
    shapes_h, merge_h = host(d_shapes, capi.SHAPE_DTYPE), host(merge8, capi.MOTION_MERGE_DTYPE)
    tree(False)
    torch.cuda.synchronize()
    plain = host(d_tree, capi.TREE_DTYPE)
    tree(True)
    torch.cuda.synchronize()
    merged = host(d_tree, capi.TREE_DTYPE)
    hmin, hmax, hrec = capi.p_tree_select_merge(shapes_h[:n], merge_h[:n], W, H, with_tree=True)
    equal = merged[:n].tobytes() == hrec.tobytes() and d_min[:n * 256].cpu().numpy().tobytes() == hmin.tobytes() and d_max[:n * 256].cpu().numpy().tobytes() == hmax.tobytes()
    print("device equals the host function on picture 0:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture 0 differs from the host function: nothing is timed")
    coded = (plain["cost_own"] != MARK) & (merged["cost_own"] != MARK)
    wins = (merged["flags"] & 64) != 0
    effect = {"coded_nodes": int(coded.sum()), "share_of_nodes_where_merge_wins": float(wins[coded].mean()),
              "share_per_level": {str(l): float(wins[coded & (merged["level"] == l)].mean()) for l in range(4)},
              "mean_own_without_merge": float(plain["cost_own"][coded].mean()), "mean_own_with_merge": float(merged["cost_own"][coded].mean())}
    tree(False)
    torch.cuda.synchronize()
    hi_plain = d_max.cpu().numpy().copy()
    tree(True)
    torch.cuda.synchronize()
    effect["share_of_units_with_smaller_depth_max"] = float((d_max.cpu().numpy() < hi_plain).mean())
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
    launches = {name: args.tree_launches if "tree" in name else args.launches for name in runs}
    for _ in range(args.repeats):     # interleaved: one window of each per round
        for name, fn in runs.items():
            ms[name].append(window(fn, launches[name]))

    out = {"tool": "tools/motion_merge_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pairs": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8"},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the six runs; ms = median of the windows",
           "device_equals_host_function_on_picture_0": bool(equal), "effect_of_the_merge_costs_at_range_8": effect, "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": launches[name]}
        print(f"{name:22s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})", flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios"] = {"a_over_b": ratio("a_merge_8", "b_refine_8"), "c_over_d": ratio("c_merge_64", "d_refine_64"),
                     "e_over_f": ratio("e_tree_with_merge", "f_tree_without_merge")}
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
