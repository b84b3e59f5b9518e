#!/usr/bin/env python3
"""Measurement: the RD stage on the device (fhevc_motion_rd_device, k_motion_rd.hip) beside the skip stage and the merge stage on the same records, and
the tree on RD costs beside the skip tree, on the bench GOP's geometry.  tools/motion_skip_bench.py's protocol.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 picture pairs = 32 130 CTUs per call.  The records are real: the SAD searches
of the nodes at range 8 and at range 64, their quarter-sample refinements, the re-pricing at range 8 and the merge stage at both ranges run once.  The
legs are timed in ONE process, interleaved (every round times each of them once, so a drift of the machine meets all alike), each as a window of warmed,
repeated launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows with the smallest
and largest next to it:
  a  the RD stage on the merge records at max_range 8         e  the RD stage on the merge records at max_range 64
  b  the RD stage on the explicit records (re-priced, with    f  the RD stage on the explicit records (refined, zero predictor) at max_range 64
     their predictor records) at max_range 8
  c  the skip stage on the merge records at max_range 8       g  the skip stage at max_range 64
     (the yardstick: the same prediction, a quarter of the
     dot products by a count of the code)
  d  fhevc_motion_merge_device at max_range 8                 h  fhevc_motion_merge_device at max_range 64
  i  the tree on the RD records, skip_mask 3 (maps, records)  j  fhevc_p_tree_select_skip_device on the same bytes
Recorded, not asserted: a / c, b / c, e / g, f / g, i / j with the run-to-run spread, and how often a depth-0 TU splits per level.  Before anything is
timed the device's RD records of picture pair 0 are compared with the host form.  Every leg's figures carry the SHA-256 of the buffers it wrote.

Needs an MI355X; without one it fails.  Writes profiles/motion_rd.json (--out)."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=5, help="launches per window of the motion legs (milliseconds each)")
    ap.add_argument("--tree-launches", type=int, default=50, help="launches per window of the two tree legs (tens of microseconds each)")
    ap.add_argument("--lib", default=None, help="another build of the library to measure (default: the tree's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_rd.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("motion_rd_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_rd_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF, lib_path=args.lib)
    n = ctx.num_ctus
    total = P * n
    pics = frames.pan_clip(W, H, NF)
    d8 = torch.from_numpy(np.stack(pics)).cuda()
    buf = lambda nbytes=16: torch.zeros((total * 85 * nbytes,), dtype=torch.uint8, device="cuda")
    found8, fine8, priced8, merge8, found64, fine64, merge64 = (buf() for _ in range(7))
    mvp8 = buf(8)
    rd_m, rd_e, scratch, d_tree = buf(), buf(), buf(), buf()
    d_min = torch.zeros((total * 256,), dtype=torch.uint8, device="cuda")
    d_max = torch.zeros_like(d_min)
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)
    p = lambda t: t.data_ptr()

    ctx.motion_search_pu_wide_device(*layout, p(found8), None, None, stream=st, qp=qp, search_range=8)
    ctx.motion_refine_device(*layout, p(found8), p(fine8), stream=st, qp=qp, max_range=8)
    ctx.motion_amvp_device(NF, p(fine8), d_out_nodes=p(priced8), d_mvp_nodes=p(mvp8), stream=st, qp=qp)
    ctx.motion_merge_device(*layout, p(priced8), p(merge8), stream=st, qp=qp, max_range=8)
    ctx.motion_search_pu_wide_device(*layout, p(found64), None, None, stream=st, qp=qp, search_range=64)
    ctx.motion_refine_device(*layout, p(found64), p(fine64), stream=st, qp=qp, max_range=64)
    ctx.motion_merge_device(*layout, p(fine64), p(merge64), stream=st, qp=qp, max_range=64)
    ctx.motion_rd_device(*layout, capi.RD_SOURCE_MERGE, p(merge8), p(rd_m), stream=st, qp=qp, max_range=8)
    ctx.motion_rd_device(*layout, capi.RD_SOURCE_EXPLICIT, p(priced8), p(rd_e), d_mvp=p(mvp8), stream=st, qp=qp, max_range=8)
    torch.cuda.synchronize()

    rd = lambda source, rec, R, mvp=None: ctx.motion_rd_device(*layout, source, p(rec), p(scratch), d_mvp=None if mvp is None else p(mvp), stream=st, qp=qp, max_range=R)
    outs = (p(d_min), p(d_max), p(d_tree))
    runs = {
        "a_rd_merge_8": lambda: rd(capi.RD_SOURCE_MERGE, merge8, 8),
        "b_rd_explicit_8": lambda: rd(capi.RD_SOURCE_EXPLICIT, priced8, 8, mvp8),
        "c_skip_8": lambda: ctx.motion_skip_device(*layout, p(merge8), p(scratch), stream=st, qp=qp, max_range=8),
        "d_merge_8": lambda: ctx.motion_merge_device(*layout, p(priced8), p(scratch), stream=st, qp=qp, max_range=8),
        "e_rd_merge_64": lambda: rd(capi.RD_SOURCE_MERGE, merge64, 64),
        "f_rd_explicit_64": lambda: rd(capi.RD_SOURCE_EXPLICIT, fine64, 64),
        "g_skip_64": lambda: ctx.motion_skip_device(*layout, p(merge64), p(scratch), stream=st, qp=qp, max_range=64),
        "h_merge_64": lambda: ctx.motion_merge_device(*layout, p(fine64), p(scratch), stream=st, qp=qp, max_range=64),
        "i_tree_rd": lambda: ctx.p_tree_select_rd_device(p(rd_e), p(rd_m), 3, P, *outs, stream=st),
        "j_tree_skip": lambda: ctx.p_tree_select_skip_device(p(rd_e), p(rd_m), p(rd_m), 3, P, *outs, stream=st),
    }
    written = {name: [d_min, d_max, d_tree] if "tree" in name else [scratch] for name in runs}   # the buffers a leg writes

    # the result first: picture pair 0 against the host form
    host = lambda t, dt: t.cpu().numpy().view(dt).reshape(total, 85)
    merge_h, rd_h = host(merge8, capi.MOTION_MERGE_DTYPE), host(rd_m, capi.MOTION_RD_DTYPE)
    host_rd = ctx.motion_rd(pics[1].astype(np.int16), pics[0].astype(np.int16), merge_h[:n], capi.RD_SOURCE_MERGE, origin=0, stride=W, qp=qp, max_range=8)
    equal = host_rd.tobytes() == rd_h[:n].tobytes()
    print("device equals the host form on picture pair 0:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture pair 0 differs from the host form: nothing is timed")
    splits = {}
    for name, rec in (("merge_8", rd_h), ("explicit_8", host(rd_e, capi.MOTION_RD_DTYPE))):
        valid = rec["cost_rd"] != MARK
        splits[name] = {}
        for l, (lo, hi) in enumerate(((0, 1), (1, 5), (5, 21), (21, 85))):
            v, t = valid[:, lo:hi], rec["tu_split"][:, lo:hi]
            tus = 4 if l == 0 else 1
            taken = sum(int(((t >> b) & 1)[v].sum()) for b in range(tus))
            splits[name][str(l)] = {"valid_nodes": int(v.sum()), "depth0_tus": int(v.sum()) * tus, "share_of_depth0_tus_split": taken / max(1, int(v.sum()) * tus),
                                    "share_of_nodes_zero_under_add_plain": float(((rec["flags"][:, lo:hi] & 1) != 0)[v].mean()) if v.any() else 0.0}
    print("splits:", json.dumps(splits), flush=True)

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

    out = {"tool": "tools/motion_rd_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library(args.lib).fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pairs": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8"},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the ten runs; ms = median of the windows",
           "device_equals_host_form_on_picture_pair_0": bool(equal), "tu_splits_per_level_at_range_8": splits,
           "expectation_from_a_count_of_the_code": "about 3 x the skip stage's dot products (forward and inverse, at N and at N / 2, where the skip stage has forward at N)",
           "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": launches[name], "sha256": sha[name]}
        print(f"{name:22s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  sha256 {sha[name][:16]}", flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios"] = {"a_over_c": ratio("a_rd_merge_8", "c_skip_8"), "b_over_c": ratio("b_rd_explicit_8", "c_skip_8"), "e_over_g": ratio("e_rd_merge_64", "g_skip_64"),
                     "f_over_g": ratio("f_rd_explicit_64", "g_skip_64"), "a_over_d": ratio("a_rd_merge_8", "d_merge_8"), "e_over_h": ratio("e_rd_merge_64", "h_merge_64"),
                     "i_over_j": ratio("i_tree_rd", "j_tree_skip")}
    print("ratios:", json.dumps(out["ratios"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
