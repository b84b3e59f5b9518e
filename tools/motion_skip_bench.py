#!/usr/bin/env python3
"""Measurement: the zero-residual stage on the device (fhevc_motion_skip_device, k_motion_skip.hip) beside the merge stage whose records it reads, and
the tree decision with and without the skip records, on the bench GOP's geometry.  tools/motion_merge_bench.py's protocol.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 picture pairs = 32 130 CTUs per call.  The records are real: the SAD searches
at range 8 (all three families) and at range 64 (the nodes), their quarter-sample refinements, the partition-size selection and the merge stage at both
ranges run once.  Six things are timed in ONE process, interleaved (every round times each of them once, so a drift of the machine meets all six alike),
each as a window of warmed, repeated launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats
windows with the smallest and largest next to it:
  a  the skip stage at max_range 8 on the merge records of range 8
  b  fhevc_motion_merge_device at max_range 8 on the nodes those came from (the yardstick: a kernel older than the skip stage)
  c  the skip stage at max_range 64
  d  fhevc_motion_merge_device at max_range 64
  e  the tree decision with the skip records, skip_mask 3 (maps and records)
  f  fhevc_p_tree_select_merge_device on the same records
Recorded, not asserted: a / b, c / d, e / f with the run-to-run spread; the share of coded nodes with each bit set, per level, at QP 22 / 27 / 32 / 37;
how often the skip rule changes depth_max.  Before anything is timed the device's skip records of picture pair 0 are compared with the host form, and the
device's skip-tree records and maps of picture 0 with the host function.  Every leg's figures carry the SHA-256 of the buffers it wrote: the inputs are
seeded, so two builds that behave alike give equal digests.  --lib times another build of the library (A/B of a kernel variant) under the same protocol.

Needs an MI355X; without one it fails.  Writes profiles/motion_skip.json (--out)."""
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
QPS = (22, 27, 32, 37)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=5, help="launches per window of the four motion legs (milliseconds each)")
    ap.add_argument("--tree-launches", type=int, default=50, help="launches per window of the two tree legs (tens of microseconds each)")
    ap.add_argument("--lib", default=None, help="another build of the library to measure (default: the tree's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_skip.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("motion_skip_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_skip_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF, lib_path=args.lib)
    n = ctx.num_ctus
    total = P * n
    pics = frames.pan_clip(W, H, NF)
    d8 = torch.from_numpy(np.stack(pics)).cuda()
    buf = lambda k: torch.zeros((total * k * 16,), dtype=torch.uint8, device="cuda")
    found = [buf(k) for k in (85, 124, 384)]
    refined = [buf(k) for k in (85, 124, 384)]
    found64, refined64 = buf(85), buf(85)
    merge8, merge64, skip8, scratch, d_shapes, d_tree = buf(85), buf(85), buf(85), buf(85), buf(85), buf(85)
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
    ctx.motion_merge_device(*layout, refined64.data_ptr(), merge64.data_ptr(), stream=st, qp=qp, max_range=64)
    ctx.motion_skip_device(*layout, merge8.data_ptr(), skip8.data_ptr(), stream=st, qp=qp, max_range=8)
    torch.cuda.synchronize()

    def tree(with_skip, mask=3):
        if with_skip:
            ctx.p_tree_select_skip_device(d_shapes.data_ptr(), merge8.data_ptr(), skip8.data_ptr(), mask, P, d_min.data_ptr(), d_max.data_ptr(), d_tree.data_ptr(), stream=st)
        else:
            ctx.p_tree_select_merge_device(d_shapes.data_ptr(), merge8.data_ptr(), P, d_min.data_ptr(), d_max.data_ptr(), d_tree.data_ptr(), stream=st)

    runs = {
        "a_skip_8": lambda: ctx.motion_skip_device(*layout, merge8.data_ptr(), scratch.data_ptr(), stream=st, qp=qp, max_range=8),
        "b_merge_8": lambda: ctx.motion_merge_device(*layout, rp[0], scratch.data_ptr(), stream=st, qp=qp, max_range=8),
        "c_skip_64": lambda: ctx.motion_skip_device(*layout, merge64.data_ptr(), scratch.data_ptr(), stream=st, qp=qp, max_range=64),
        "d_merge_64": lambda: ctx.motion_merge_device(*layout, refined64.data_ptr(), scratch.data_ptr(), stream=st, qp=qp, max_range=64),
        "e_tree_with_skip": lambda: tree(True),
        "f_tree_with_merge": lambda: tree(False),
    }
    written = {name: [d_min, d_max, d_tree] if "tree" in name else [scratch] for name in runs}   # the buffers a leg writes

    # the result first: picture pair 0 against the host form, picture 0's tree against the host function
    host = lambda t, dt: t.cpu().numpy().view(dt).reshape(total, 85)
    shapes_h, merge_h, skip_h = host(d_shapes, capi.SHAPE_DTYPE), host(merge8, capi.MOTION_MERGE_DTYPE), host(skip8, capi.MOTION_SKIP_DTYPE)
    host_skip = ctx.motion_skip(pics[1].astype(np.int16), pics[0].astype(np.int16), merge_h[:n], 0, W, qp=qp, max_range=8)
    tree(True)
    torch.cuda.synchronize()
    skipped = host(d_tree, capi.TREE_DTYPE)
    hmin, hmax, hrec = capi.p_tree_select_skip(shapes_h[:n], merge_h[:n], skip_h[:n], 3, W, H, with_tree=True)
    equal = (host_skip.tobytes() == skip_h[:n].tobytes() and skipped[:n].tobytes() == hrec.tobytes() and d_min[:n * 256].cpu().numpy().tobytes() == hmin.tobytes()
             and d_max[:n * 256].cpu().numpy().tobytes() == hmax.tobytes())
    print("device equals the host path on picture 0:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture 0 differs from the host path: nothing is timed")
    hi_skip = d_max.cpu().numpy().copy()
    tree(False)
    torch.cuda.synchronize()
    merged = host(d_tree, capi.TREE_DTYPE)
    hi_merge = d_max.cpu().numpy().copy()
    coded = merged["cost_own"] != MARK
    effect = {"coded_nodes": int(coded.sum()), "share_of_coded_nodes_whose_own_cost_is_the_merge_cost": float(((merged["flags"] & 64) != 0)[coded].mean()),
              "nodes_of_level_0_to_2_not_descended_at_mask_3": int(((skipped["flags"] & 128) != 0).sum()),
              "share_of_units_with_smaller_depth_max_at_mask_3": float((hi_skip < hi_merge).mean()),
              "share_of_ctus_whose_depth_max_changes_at_mask_3": float((hi_skip.reshape(total, 256) != hi_merge.reshape(total, 256)).any(axis=1).mean())}
    bits = {}
    for q in QPS:
        ctx.motion_skip_device(*layout, merge8.data_ptr(), scratch.data_ptr(), stream=st, qp=q, max_range=8)
        torch.cuda.synchronize()
        rec = host(scratch, capi.MOTION_SKIP_DTYPE)
        valid = rec["coef_max"] != MARK
        bits[str(q)] = {str(l): {"valid_nodes": int(valid[:, lo:hi].sum()), "bit0_zero_under_add_plain": float(((rec["flags"] & 1) != 0)[:, lo:hi][valid[:, lo:hi]].mean()),
                                 "bit1_zero_under_add_half": float(((rec["flags"] & 2) != 0)[:, lo:hi][valid[:, lo:hi]].mean())}
                        for l, (lo, hi) in enumerate(((0, 1), (1, 5), (5, 21), (21, 85)))}
    print("effect:", json.dumps(effect), flush=True)
    print("bits:", json.dumps(bits), flush=True)

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
    sha = {}
    for name, fn in runs.items():     # one more launch of each, alone, and what it left behind
        fn()
        torch.cuda.synchronize()
        sha[name] = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in written[name])).hexdigest()

    out = {"tool": "tools/motion_skip_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library(args.lib).fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pairs": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8"},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the six runs; ms = median of the windows",
           "device_equals_host_path_on_picture_0": bool(equal), "effect_of_the_skip_rule_at_range_8": effect,
           "share_of_valid_nodes_with_each_bit_per_qp_and_level": bits, "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": launches[name], "sha256": sha[name]}
        print(f"{name:22s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  sha256 {sha[name][:16]}", flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios"] = {"a_over_b": ratio("a_skip_8", "b_merge_8"), "c_over_d": ratio("c_skip_64", "d_merge_64"), "e_over_f": ratio("e_tree_with_skip", "f_tree_with_merge")}
    print("ratios:", json.dumps(out["ratios"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
