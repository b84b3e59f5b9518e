#!/usr/bin/env python3
"""Measurement: the RD stages at three TU depths (fhevc_motion_rd_qt_device, fhevc_motion_rd_pu_qt_device with tu_depths 3: further instances of
k_motion_rd.hip) beside the RD stage at two depths on the same nodes (fhevc_motion_rd_device, whose code this change leaves as it was), on the bench GOP's
geometry.  tools/motion_rd_pu_bench.py's protocol.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 picture pairs = 32 130 CTUs per call.  The records are real, per range 8 and
64: the SAD searches of all three families, their quarter-sample refinements, the re-pricing with its predictor records, the merge stages of the nodes
and of the PUs and the merge-aware selection run once.  The legs are timed in ONE process, interleaved (every round times each of them once), each as a
window of warmed, repeated launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows
with the smallest and largest next to it.  Per max_range R in {8, 64}:
  y    the yardstick: fhevc_motion_rd_device on the re-priced nodes with their predictor records
  q3   the same nodes through fhevc_motion_rd_qt_device at tu_depths 3
  p0_2 / p0_3, p8_2 / p8_3   the PU form at part_mode 0 and 8 (the selection's best), at 2 and at 3 depths
  seq_2 / seq_3              the three launches 0, 8 folded, 9 folded on one stream, at 2 and at 3 depths
Recorded, not asserted: every leg as a ratio to y with the run-to-run spread, beside the expectation from a count of the code (about a quarter more
transform work); per level 1 / 2 the share of valid nodes whose cost falls and rises against two depths and the share with some depth-1 split; how many
entries of the RD tree's depth maps change and the mean depth_max before and after; what the occupancy query answers for the MR = 64 instances.  Before
anything is timed the device's records of picture pair 0 at three depths are compared with the host form.  Quality (BD-rate) is not measured.

Needs an MI355X; without one it fails.  Writes profiles/motion_rd_qt.json (--out)."""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_rd_qt.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("motion_rd_qt_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_rd_qt_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF)
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

    # what the device keeps resident of the MR = 64 instances
    lib = ctx.lib
    lib.fhevc_debug_motion_rd_wide_residency.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    residency = {}
    for pu_form in (0, 1):
        for tud in (2, 3):
            per_cu = C.c_int(0)
            assert lib.fhevc_debug_motion_rd_wide_residency(ctx.h, 1, pu_form, tud, C.byref(per_cu)) == capi.OK
            residency[f"{'pu' if pu_form else 'plain'}_uint8_MR64_tu_depths_{tud}"] = {"workgroups_per_cu_by_the_occupancy_query": per_cu.value, "dynamic_lds_bytes": 80016,
                                                                                    "static_lds_bytes": 1824, "threads": 256}
    print("residency:", json.dumps(residency), flush=True)

    chain = {}
    for R in (8, 64):
        found, fine, priced = [buf(f) for f in FAM], [buf(f) for f in FAM], [buf(f) for f in FAM]
        mvp = [buf(f, 8) for f in FAM]
        merge, merge_pu, merge_s, shapes = buf(), buf(124), buf(384), buf()
        ctx.motion_search_pu_wide_device(*layout, *[p(t) for t in found], stream=st, qp=qp, search_range=R)
        ctx.motion_refine_pu_wide_device(*layout, p(found[0]), p(fine[0]), p(found[1]), p(fine[1]), p(found[2]), p(fine[2]), stream=st, qp=qp, max_range=R)
        ctx.motion_amvp_device(NF, *[p(t) for t in fine], *[p(t) for t in priced], *[p(t) for t in mvp], stream=st, qp=qp)
        ctx.motion_merge_device(*layout, p(priced[0]), p(merge), stream=st, qp=qp, max_range=R)
        ctx.motion_merge_pu_device(*layout, p(priced[0]), p(merge_pu), p(merge_s), stream=st, qp=qp, max_range=R)
        ctx.pu_shape_select_merge_device(*[p(t) for t in priced], p(merge_pu), p(merge_s), P, p(shapes), stream=st)
        torch.cuda.synchronize()
        del found, fine
        chain[R] = dict(priced=priced, mvp=mvp, merge=merge, merge_pu=merge_pu, merge_s=merge_s, shapes=shapes,
                        inputs=lambda fold=None, q=priced, m=(merge_pu, merge_s), v=mvp, s=shapes: ctx.rd_pu_inputs(p(q[0]), p(q[1]), p(q[2]), p(m[0]), p(m[1]), p(v[0]), p(v[1]),
                                                                                                                  p(v[2]), p(s), fold))
    scratch, folded, rd_merge = buf(), buf(), buf()
    pu_launch = lambda R, mode, tud, out, fold=None: ctx.motion_rd_pu_qt_device(*layout, mode, chain[R]["inputs"](fold), tud, p(out), stream=st, qp=qp, max_range=R)

    def sequence(R, tud, out):
        pu_launch(R, 0, tud, out)
        pu_launch(R, 8, tud, out, p(out))
        pu_launch(R, 9, tud, out, p(out))

    # the result first: picture pair 0 of the folded sequence at three depths and range 8 against the host form, launch by launch
    sequence(8, 3, folded)
    torch.cuda.synchronize()
    host = lambda t, dt, per=85: t.cpu().numpy().view(dt).reshape(total, per)
    c8 = chain[8]
    arrays = [host(t, capi.MOTION_QPEL_DTYPE, f)[:n] for t, f in zip(c8["priced"], FAM)] + [host(c8["merge_pu"], capi.MOTION_MERGE_DTYPE, 124)[:n],
              host(c8["merge_s"], capi.MOTION_MERGE_DTYPE, 384)[:n]] + [host(t, capi.MOTION_MVP_DTYPE, f)[:n] for t, f in zip(c8["mvp"], FAM)] + [
              host(c8["shapes"], capi.SHAPE_DTYPE)[:n]]
    cur, ref = pics[1].astype(np.int16), pics[0].astype(np.int16)
    h = ctx.motion_rd_pu_qt(cur, ref, 0, arrays[0], 3, *arrays[1:], origin=0, stride=W, qp=qp, max_range=8)
    for mode in (8, 9):
        h = ctx.motion_rd_pu_qt(cur, ref, mode, arrays[0], 3, *arrays[1:], fold=h, origin=0, stride=W, qp=qp, max_range=8)
    equal = h.tobytes() == host(folded, capi.MOTION_RD_PU_DTYPE)[:n].tobytes()
    ctx.motion_rd_qt_device(*layout, capi.RD_SOURCE_EXPLICIT, p(c8["priced"][0]), 3, p(scratch), d_mvp=p(c8["mvp"][0]), stream=st, qp=qp, max_range=8)
    torch.cuda.synchronize()
    hp = ctx.motion_rd_qt(cur, ref, arrays[0], capi.RD_SOURCE_EXPLICIT, 3, mvp=arrays[5], origin=0, stride=W, qp=qp, max_range=8)
    equal = equal and hp.tobytes() == host(scratch, capi.MOTION_RD_DTYPE)[:n].tobytes()
    print("device equals the host form on picture pair 0:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture pair 0 differs from the host form: nothing is timed")

    # what the third depth changes: costs per level, depth-1 splits, the RD tree's maps
    effect = {}
    d_min, d_max = (torch.zeros((total * 256,), dtype=torch.uint8, device="cuda") for _ in range(2))
    for R in (8, 64):
        recs, maps = {}, {}
        for tud in (2, 3):
            sequence(R, tud, folded)
            ctx.motion_rd_qt_device(*layout, capi.RD_SOURCE_MERGE, p(chain[R]["merge"]), tud, p(rd_merge), stream=st, qp=qp, max_range=R)
            ctx.p_tree_select_rd_pu_device(p(folded), p(rd_merge), 3, P, p(d_min), p(d_max), stream=st)
            torch.cuda.synchronize()
            recs[tud] = host(folded, capi.MOTION_RD_PU_DTYPE).copy()
            maps[tud] = (d_min.cpu().numpy().copy(), d_max.cpu().numpy().copy())
        per_level = {}
        for l in (1, 2):
            lo, hi = LEVELS[l]
            a, b = recs[2][:, lo:hi], recs[3][:, lo:hi]
            v = a["part"] != 255
            ca, cb = a["cost_rd"][v].astype(np.int64), b["cost_rd"][v].astype(np.int64)
            per_level[str(l)] = {"valid_nodes": int(v.sum()), "share_cost_down": float((cb < ca).mean()), "share_cost_up": float((cb > ca).mean()),
                                 "share_with_some_depth_1_split": float(((b["tu_split"][v] & 0xF0) != 0).mean()),
                                 "share_depth_0_split_at_2": float(((a["tu_split"][v] & 1) != 0).mean()), "share_depth_0_split_at_3": float(((b["tu_split"][v] & 1) != 0).mean())}
        effect[str(R)] = {"folded_records_per_level": per_level,
                          "rd_tree": {"depth_min_entries_changed": int((maps[2][0] != maps[3][0]).sum()), "depth_max_entries_changed": int((maps[2][1] != maps[3][1]).sum()),
                                      "entries": int(maps[2][1].size), "mean_depth_max_at_2": float(maps[2][1].mean()), "mean_depth_max_at_3": float(maps[3][1].mean()),
                                      "mean_depth_min_at_2": float(maps[2][0].mean()), "mean_depth_min_at_3": float(maps[3][0].mean())}}
    print("effect:", json.dumps(effect), flush=True)

    runs = {}
    for R in (8, 64):
        c = chain[R]
        runs[f"y_rd_explicit_{R}"] = lambda R=R, c=c: ctx.motion_rd_device(*layout, capi.RD_SOURCE_EXPLICIT, p(c["priced"][0]), p(scratch), d_mvp=p(c["mvp"][0]), stream=st, qp=qp,
                                                                          max_range=R)
        runs[f"q3_{R}"] = lambda R=R, c=c: ctx.motion_rd_qt_device(*layout, capi.RD_SOURCE_EXPLICIT, p(c["priced"][0]), 3, p(scratch), d_mvp=p(c["mvp"][0]), stream=st, qp=qp,
                                                                   max_range=R)
        for mode in (0, 8):
            for tud in (2, 3):
                runs[f"p{mode}_{tud}_{R}"] = lambda R=R, mode=mode, tud=tud: pu_launch(R, mode, tud, scratch)
        for tud in (2, 3):
            runs[f"seq_{tud}_{R}"] = lambda R=R, tud=tud: sequence(R, tud, folded)

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
    for _ in range(args.repeats):     # interleaved: one window of each per round
        for name, fn in runs.items():
            ms[name].append(window(fn, args.launches))
    sha = {}
    for name, fn in runs.items():     # one more launch of each, alone, and what it left behind
        fn()
        torch.cuda.synchronize()
        sha[name] = hashlib.sha256((folded if name.startswith("seq") else scratch).cpu().numpy().tobytes()).hexdigest()

    out = {"tool": "tools/motion_rd_qt_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pairs": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8"},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the runs; ms = median of the windows; seq: ms per "
                     "sequence of three launches",
           "device_equals_host_form_on_picture_pair_0": bool(equal), "residency": residency, "what_the_third_depth_changes": effect, "quality_bd_rate": "not measured",
           "expectation_from_a_count_of_the_code": "four more passes over two of the four buffers: about a quarter more transform work than two depths, so q3 / y about 1.25 "
                                                   "at equal residency (an expectation only)",
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
    out["ratios_three_depths_to_two"] = {f"{leg}_{R}": ratio(f"{leg}_3_{R}", f"{leg}_2_{R}") for leg in ("p0", "p8", "seq") for R in (8, 64)}
    print("ratios:", json.dumps(out["ratios_to_the_yardstick"]), flush=True)
    print("three to two:", json.dumps(out["ratios_three_depths_to_two"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
