#!/usr/bin/env python3
"""Measurement: the RD estimate of the intra candidate at three TU depths (fhevc_intra_rd_qt_device with tu_depths 3: the two further intra instances of
k_motion_rd.hip) against the same stage at two (fhevc_intra_rd_device, the instances there were) on the same records.  tools/intra_rd_bench.py's protocol.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): pictures 1..63 = 32 130 CTUs per call.  The records are real, at range 8: the chain
of fhevc_p_tree_rd_qt_frame at tu_depths 3 up to the folded inter records (part_mode 0, 8, 9) and the merge records' RD records run once, and so does the
first pass of pictures 1..63.  The legs are timed in ONE process, interleaved (every round times each of them once), each as a window of warmed, repeated
launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows with the smallest and largest
next to it:
  two    fhevc_intra_rd_device, plain
  three  fhevc_intra_rd_qt_device at tu_depths 3, plain
  fold2 / fold3   the same two with the calm gate (skip_mask 3) and the fold in place into a copy of the inter records folded at three depths
Recorded, not asserted: three against two as a ratio with the run-to-run spread, beside a count of the added work; per level how often the cost falls and
rises against two depths, how often some depth-1 TU splits, how often intra wins the fold at 3 against at 2 (both on records folded at 3); how many entries
of the RD tree's depth maps change and the mean depth_max.  Before anything is timed the device's records of picture 1 are compared with the host form.
Quality (BD-rate): not measured.

Needs an MI355X; without one it fails.  Writes profiles/intra_rd_qt.json (--out)."""
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
# transform passes over one level's buffer (64 x 64 samples each) per CTU: two depths run 2 depths x 4 levels, three depths add one depth on two levels; the
# third prediction adds one pass over two levels (and makes the level-3 one real) to 2 x 4; the 4x4 lines add 256 x 17 samples to 3 925 x 2
ADDED_WORK = {"transform_buffer_passes": [8, 10], "prediction_level_passes": [8, 10], "line_samples": [7850, 12202]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=5, help="launches per window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_rd_qt.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("intra_rd_qt_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("intra_rd_qt_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, R, mask = args.width, args.height, args.frames, args.qp, 8, 3
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
    current = (d8.data_ptr() + W * H, 1, W, W * H, P)   # pictures 1..63: the current picture of every pair
    p = lambda t: t.data_ptr()
    FAM = (85, 124, 384)

    # the inter chain at three TU depths, once: what fhevc_p_tree_rd_qt_frame queues, on the batch
    found, fine, priced = [buf(f) for f in FAM], [buf(f) for f in FAM], [buf(f) for f in FAM]
    mvp = [buf(f, 8) for f in FAM]
    merge, merge_pu, merge_s, shapes, rd_merge, inter = buf(), buf(124), buf(384), buf(), buf(), buf()
    ctx.motion_search_pu_wide_device(*layout, *[p(t) for t in found], stream=st, qp=qp, search_range=R)
    ctx.motion_refine_pu_wide_device(*layout, p(found[0]), p(fine[0]), p(found[1]), p(fine[1]), p(found[2]), p(fine[2]), stream=st, qp=qp, max_range=R)
    ctx.motion_amvp_device(NF, *[p(t) for t in fine], *[p(t) for t in priced], *[p(t) for t in mvp], stream=st, qp=qp)
    ctx.motion_merge_device(*layout, p(priced[0]), p(merge), stream=st, qp=qp, max_range=R)
    ctx.motion_merge_pu_device(*layout, p(priced[0]), p(merge_pu), p(merge_s), stream=st, qp=qp, max_range=R)
    ctx.pu_shape_select_merge_device(*[p(t) for t in priced], p(merge_pu), p(merge_s), P, p(shapes), stream=st)
    ctx.motion_rd_qt_device(*layout, capi.RD_SOURCE_MERGE, p(merge), 3, p(rd_merge), stream=st, qp=qp, max_range=R)
    for mode in (0, 8, 9):
        inputs = ctx.rd_pu_inputs(p(priced[0]), p(priced[1]), p(priced[2]), p(merge_pu), p(merge_s), p(mvp[0]), p(mvp[1]), p(mvp[2]), p(shapes), p(inter) if mode else None)
        ctx.motion_rd_pu_qt_device(*layout, mode, inputs, 3, p(inter), stream=st, qp=qp, max_range=R)
    first = buf()
    ctx.intra_first_pass_device(*current, p(first), stream=st, qp=qp)
    torch.cuda.synchronize()
    del found, fine
    plain = {2: buf(), 3: buf()}
    folded = {2: buf(), 3: buf()}

    def stage(tud, out, fold=None, m=None, k=0):
        if tud == 2:
            ctx.intra_rd_device(*current, p(first), p(out), d_fold=fold, d_rd_merge=m, skip_mask=k, stream=st, qp=qp)
        else:
            ctx.intra_rd_qt_device(*current, p(first), tud, p(out), d_fold=fold, d_rd_merge=m, skip_mask=k, stream=st, qp=qp)

    # the result first: picture 1 against the host form, plain and gated + folded, at both depth counts
    host = lambda t, dt: t.cpu().numpy().view(dt).reshape(total, 85)
    for tud in (2, 3):
        stage(tud, plain[tud])
        folded[tud].copy_(inter)
        stage(tud, folded[tud], p(folded[tud]), p(rd_merge), mask)
    torch.cuda.synchronize()
    h_first, h_inter, h_merge = host(first, capi.NODE_DTYPE), host(inter, capi.MOTION_RD_PU_DTYPE), host(rd_merge, capi.MOTION_RD_DTYPE)
    h_plain = {t: host(plain[t], capi.MOTION_RD_PU_DTYPE) for t in (2, 3)}
    h_folded = {t: host(folded[t], capi.MOTION_RD_PU_DTYPE) for t in (2, 3)}
    cur = pics[1].astype(np.int16)
    equal = all(ctx.intra_rd_qt(cur, h_first[:n], t, origin=0, stride=W, qp=qp).tobytes() == h_plain[t][:n].tobytes() and
                ctx.intra_rd_qt(cur, h_first[:n], t, fold=h_inter[:n], rd_merge=h_merge[:n], skip_mask=mask, origin=0, stride=W, qp=qp).tobytes() == h_folded[t][:n].tobytes()
                for t in (2, 3))
    print("device equals the host form on picture 1:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture 1 differs from the host form: nothing is timed")

    # what the third depth changes, and what the tree makes of it
    d_min, d_max = (torch.zeros((total * 256,), dtype=torch.uint8, device="cuda") for _ in range(2))
    maps = {}
    for t in (2, 3):
        ctx.p_tree_select_rd_pu_device(p(folded[t]), p(rd_merge), mask, P, p(d_min), p(d_max), stream=st)
        torch.cuda.synchronize()
        maps[t] = (d_min.cpu().numpy().copy(), d_max.cpu().numpy().copy())
    per_level = {}
    for l, (lo, hi) in enumerate(LEVELS):
        v = h_plain[3]["part"][:, lo:hi] != 255
        c2, c3 = (h_plain[t]["cost_rd"][:, lo:hi].astype(np.int64) for t in (2, 3))
        share = lambda m: float(m[v].mean()) if v.any() else 0.0
        per_level[str(l)] = {"valid_nodes": int(v.sum()), "share_cost_falls": share(c3 < c2), "share_cost_rises": share(c3 > c2),
                             "share_depth_0_split_at_3": share(h_plain[3]["tu_split"][:, lo:hi] & (15 if l == 0 else 1) != 0),
                             "share_depth_0_split_at_2": share(h_plain[2]["tu_split"][:, lo:hi] & (15 if l == 0 else 1) != 0),
                             "share_some_depth_1_tu_splits": share(h_plain[3]["tu_split"][:, lo:hi] >> 4 != 0),
                             "share_intra_wins_the_fold_at_3": share(h_folded[3]["part"][:, lo:hi] == capi.RD_PART_INTRA),
                             "share_intra_wins_the_fold_at_2": share(h_folded[2]["part"][:, lo:hi] == capi.RD_PART_INTRA)}
    choice = {"per_level": per_level, "both_folds_into": "the inter records folded at tu_depths 3",
              "depth_maps_intra_at_3_against_intra_at_2": {
                  "share_of_depth_min_entries_changed": float((maps[3][0] != maps[2][0]).mean()), "share_of_depth_max_entries_changed": float((maps[3][1] != maps[2][1]).mean()),
                  "mean_depth_max_intra_at_3": float(maps[3][1].mean()), "mean_depth_max_intra_at_2": float(maps[2][1].mean())}}
    print("choice:", json.dumps(choice), flush=True)

    runs = {
        "two": lambda: stage(2, plain[2]),
        "three": lambda: stage(3, plain[3]),
        "fold2": lambda: stage(2, folded[2], p(folded[2]), p(rd_merge), mask),
        "fold3": lambda: stage(3, folded[3], p(folded[3]), p(rd_merge), mask),
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
    where = {"two": plain[2], "three": plain[3], "fold2": folded[2], "fold3": folded[3]}
    sha = {name: hashlib.sha256(where[name].cpu().numpy().tobytes()).hexdigest() for name in runs}

    out = {"tool": "tools/intra_rd_qt_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pictures_priced": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8", "max_range": R},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the runs; ms = median of the windows",
           "device_equals_host_form_on_picture_1": bool(equal), "what_the_third_depth_changes": choice, "quality_bd_rate": "not measured",
           "added_work_by_a_count_of_the_code_two_against_three_depths": ADDED_WORK, "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": args.launches, "sha256": sha[name]}
        print(f"{name:8s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  sha256 {sha[name][:16]}", flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["three_against_two"] = {"plain": ratio("three", "two"), "gated_and_folded": ratio("fold3", "fold2")}
    print("three against two:", json.dumps(out["three_against_two"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
