#!/usr/bin/env python3
"""Measurement: the tree decision on the device (fhevc_p_tree_select_device, k_p_tree.hip) on the bench GOP's geometry.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 P pictures = 32 130 CTUs per call.  The records are real: the SAD searches
of all three families at --range (default 8), their quarter-sample refinement and the partition-size selection run once, the tree reads that output.
Four things are timed in ONE process, interleaved (every round times each of them once, so a drift of the machine meets all four alike), each as a
window of warmed, repeated launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows
with the smallest and largest next to it:
  a  the tree with all three outputs (reads 1 360 B of records per CTU, writes 512 B of maps and 1 360 B of tree records)
  b  the maps only (writes 512 B)
  c  fhevc_pu_shape_select_device without the cost table, on the entries the records came from (reads 9 488 B per CTU, writes 1 360 B)
  d  a device-to-device hipMemcpyAsync of the 1 360 B of records per CTU: the yardstick for a pass that must read those bytes once (the copy moves
     them twice, a read and a write)
Recorded, not asserted: a / c, b / c, b / d with the run-to-run spread (the smallest and largest ratio of windows of the same round).  Before anything
is timed the device maps and tree records of picture 0 are compared with the host function.

Needs an MI355X; without one it fails.  Writes profiles/p_tree.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fasthevc_amd import capi, frames  # noqa: E402

IN_BYTES = (85 + 124 + 384) * 16       # 9 488 per CTU: what the selection reads
REC_BYTES, MAP_BYTES = 85 * 16, 512


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--range", type=int, default=8, help="search range of the searches and max_range of the refinement (1..64)")
    ap.add_argument("--repeats", type=int, default=9, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=50, help="launches per window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p_tree.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("p_tree_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("p_tree_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, R = args.width, args.height, args.frames, args.qp, args.range
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    total = P * n
    d8 = torch.from_numpy(np.stack(frames.pan_clip(W, H, NF))).cuda()
    per = (85, 124, 384)
    found = [torch.zeros((total, k, 16), dtype=torch.uint8, device="cuda") for k in per]
    refined = [torch.zeros((total, k, 16), dtype=torch.uint8, device="cuda") for k in per]
    d_shapes = torch.zeros((total * REC_BYTES,), dtype=torch.uint8, device="cuda")
    d_shapes_again = torch.zeros_like(d_shapes)      # where the timed selection writes: the tree's input stays as it is
    copy_dst = torch.zeros_like(d_shapes)
    d_tree = torch.zeros((total * REC_BYTES,), dtype=torch.uint8, device="cuda")
    d_min = torch.zeros((total * 256,), dtype=torch.uint8, device="cuda")
    d_max = torch.zeros_like(d_min)
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)
    fp = [t.data_ptr() for t in found]
    rp = [t.data_ptr() for t in refined]
    shape_rule = capi.pu_shape_rule_default()
    tree_rule = capi.p_tree_rule(32, 0, 32, 0, 0)    # margins of an eighth, so that the two maps differ; the kernel's work does not depend on the rule

    ctx.motion_search_pu_wide_device(*layout, fp[0], fp[1], fp[2], stream=st, qp=qp, search_range=R)
    ctx.motion_refine_pu_wide_device(*layout, fp[0], rp[0], fp[1], rp[1], fp[2], rp[2], stream=st, qp=qp, max_range=R)
    ctx.pu_shape_select_device(rp[0], rp[1], rp[2], P, d_shapes.data_ptr(), None, stream=st, rule=shape_rule)
    torch.cuda.synchronize()

    def tree_all():
        ctx.p_tree_select_device(d_shapes.data_ptr(), P, d_min.data_ptr(), d_max.data_ptr(), d_tree.data_ptr(), stream=st, rule=tree_rule)

    def tree_maps():
        ctx.p_tree_select_device(d_shapes.data_ptr(), P, d_min.data_ptr(), d_max.data_ptr(), None, stream=st, rule=tree_rule)

    def select_alone():
        ctx.pu_shape_select_device(rp[0], rp[1], rp[2], P, d_shapes_again.data_ptr(), None, stream=st, rule=shape_rule)

    def copy_records():
        copy_dst.copy_(d_shapes, non_blocking=True)      # hipMemcpyAsync, device to device, on the current stream

    # the result first: picture 0 against the host function
    tree_all()
    torch.cuda.synchronize()
    host_in = d_shapes[:n * REC_BYTES].cpu().numpy().view(capi.SHAPE_DTYPE).reshape(n, 85)
    hmin, hmax, hrec = capi.p_tree_select(host_in, W, H, tree_rule, with_tree=True)
    equal = (d_min[:n * 256].cpu().numpy().tobytes() == hmin.tobytes() and d_max[:n * 256].cpu().numpy().tobytes() == hmax.tobytes() and
             d_tree[:n * REC_BYTES].cpu().numpy().tobytes() == hrec.tobytes())
    depths = {name: dict(zip(*(a.tolist() for a in np.unique(m, return_counts=True)))) for name, m in (("depth_min", hmin), ("depth_max", hmax))}
    print("device equals the host function on picture 0:", equal, " depths:", depths, flush=True)
    if not equal:
        sys.exit("the device output of picture 0 differs from the host function: nothing is timed")

    runs = {"a_tree_all_outputs": tree_all, "b_tree_maps_only": tree_maps, "c_select": select_alone, "d_copy_of_the_records": copy_records}

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    for fn in runs.values():      # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(args.repeats):     # interleaved: one window of each per round
        for name, fn in runs.items():
            ms[name].append(window(fn, args.launches))

    moved = {"a_tree_all_outputs": REC_BYTES + MAP_BYTES + REC_BYTES, "b_tree_maps_only": REC_BYTES + MAP_BYTES, "c_select": IN_BYTES + REC_BYTES,
             "d_copy_of_the_records": 2 * REC_BYTES}
    out = {"tool": "tools/p_tree_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "p_pictures": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "range": R, "planes": "uint8",
                        "record_bytes_per_ctu": REC_BYTES},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the four runs; ms = median of the windows",
           "device_equals_host_function_on_picture_0": bool(equal), "depths_of_picture_0": {k: {str(d): c for d, c in v.items()} for k, v in depths.items()},
           "runs": {}}
    for name in runs:
        v = ms[name]
        nbytes = total * moved[name]
        r = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v), "launches_per_window": args.launches,
             "bytes_from_shapes": nbytes, "bytes_per_ctu": moved[name], "tb_per_s": nbytes / (statistics.median(v) * 1e-3) / 1e12}
        out["runs"][name] = r
        print(f"{name:22s}: {r['ms'] * 1e3:10.1f} us  ({r['ms_min'] * 1e3:.1f} .. {r['ms_max'] * 1e3:.1f})  {r['tb_per_s']:.2f} TB/s from shapes", flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios"] = {"a_over_c": ratio("a_tree_all_outputs", "c_select"), "b_over_c": ratio("b_tree_maps_only", "c_select"),
                     "b_over_d": ratio("b_tree_maps_only", "d_copy_of_the_records")}
    out["expectation_recorded_not_asserted"] = {"b_below_c": out["ratios"]["b_over_c"]["ratio_of_medians"] < 1.0}
    print("ratios:", json.dumps(out["ratios"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
