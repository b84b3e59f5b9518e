#!/usr/bin/env python3
"""Measurement: the intra RD stage with the NxN candidate of the 8x8 nodes (fhevc_intra_rd_nxn_device: the two NxN instances of k_motion_rd.hip) against
the same stage without it (fhevc_intra_rd_qt_device at tu_depths 3) on the same records, and the 4x4 first pass it needs.  tools/intra_rd_qt_bench.py's
protocol.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): pictures 1..63 = 32 130 CTUs per call.  The records are real, at range 8: the chain
of fhevc_p_tree_rd_qt_frame at tu_depths 3 up to the folded inter records (part_mode 0, 8, 9) and the merge records' RD records run once, and so do the two
first passes of pictures 1..63.  The legs are timed in ONE process, interleaved (every round times each of them once), each as a window of warmed, repeated
launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows with the smallest and largest
next to it:
  nxn      (a) fhevc_intra_rd_nxn_device with d_first4 and d_nxn, plain
  nxn_fold (b) the same with the calm gate (skip_mask 3) and the fold in place into a copy of the inter records folded at three depths
  three    (c) fhevc_intra_rd_qt_device at tu_depths 3, plain, on the same records
  first4   (d) fhevc_intra_first_pass_4x4_device, best records only
Recorded, not asserted: a / c and (a + d) / c with the run-to-run spread, beside a count of the added work; how often NxN is valid and wins per picture, how
often it survives the fold; how many entries of the RD tree's depth maps change and the mean depth_max against the stage without the candidate.  Before
anything is timed the device's records of picture 1 are compared with the host form.  Quality (BD-rate): not measured.

Needs an MI355X; without one it fails.  Writes profiles/intra_rd_nxn.json (--out)."""
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

# transform passes over one level's buffer per CTU: three depths run 10, the candidate adds the level-3 buffer to the third depth; its prediction is four
# quarter-tile calls on one of the four waves
ADDED_WORK = {"transform_buffer_passes": [10, 11], "prediction_wave_passes": [10, 11], "records_read_per_ctu": [85, 85 + 256]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=5, help="launches per window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_rd_nxn.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("intra_rd_nxn_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("intra_rd_nxn_bench.py needs an MI355X: no GPU is visible")
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
    first, first4 = buf(), buf(256)
    ctx.intra_first_pass_device(*current, p(first), stream=st, qp=qp)
    first_pass_4x4 = lambda: ctx.intra_first_pass_4x4_device(*current, p(first4), None, stream=st, qp=qp, num_candidates=0)
    first_pass_4x4()
    torch.cuda.synchronize()
    del found, fine
    plain = {"three": buf(), "nxn": buf()}
    folded = {"three": buf(), "nxn": buf()}
    cand, cand_f = buf(64), buf(64)

    def stage(kind, out, fold=None, m=None, k=0, x=None):
        if kind == "three":
            ctx.intra_rd_qt_device(*current, p(first), 3, p(out), d_fold=fold, d_rd_merge=m, skip_mask=k, stream=st, qp=qp)
        else:
            ctx.intra_rd_nxn_device(*current, p(first), p(first4), p(out), p(x), d_fold=fold, d_rd_merge=m, skip_mask=k, stream=st, qp=qp)

    # the result first: picture 1 against the host form, plain and gated + folded
    for kind, x, xf in (("three", None, None), ("nxn", cand, cand_f)):
        stage(kind, plain[kind], x=x)
        folded[kind].copy_(inter)
        stage(kind, folded[kind], p(folded[kind]), p(rd_merge), mask, x=xf)
    torch.cuda.synchronize()
    host = lambda t, dt, per=85: t.cpu().numpy().view(dt).reshape(total, per)
    h_first, h_first4 = host(first, capi.NODE_DTYPE), host(first4, capi.NODE_DTYPE, 256)
    h_inter, h_merge = host(inter, capi.MOTION_RD_PU_DTYPE), host(rd_merge, capi.MOTION_RD_DTYPE)
    h_plain = {k: host(plain[k], capi.MOTION_RD_PU_DTYPE) for k in plain}
    h_folded = {k: host(folded[k], capi.MOTION_RD_PU_DTYPE) for k in folded}
    h_cand = host(cand, capi.INTRA_RD_NXN_DTYPE, 64)
    cur = pics[1].astype(np.int16)
    hp, hx = ctx.intra_rd_nxn(cur, h_first[:n], h_first4[:n], origin=0, stride=W, qp=qp, with_nxn=True)
    hf = ctx.intra_rd_nxn(cur, h_first[:n], h_first4[:n], fold=h_inter[:n], rd_merge=h_merge[:n], skip_mask=mask, origin=0, stride=W, qp=qp)
    h3 = ctx.intra_rd_nxn(cur, h_first[:n], None, origin=0, stride=W, qp=qp)
    equal = (hp.tobytes() == h_plain["nxn"][:n].tobytes() and hx.tobytes() == h_cand[:n].tobytes() and hf.tobytes() == h_folded["nxn"][:n].tobytes() and
             h3.tobytes() == h_plain["three"][:n].tobytes() and cand.cpu().numpy().tobytes() == cand_f.cpu().numpy().tobytes())
    print("device equals the host form on picture 1:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture 1 differs from the host form: nothing is timed")

    # what the candidate changes, and what the tree makes of it
    d_min, d_max = (torch.zeros((total * 256,), dtype=torch.uint8, device="cuda") for _ in range(2))
    maps = {}
    for k in folded:
        ctx.p_tree_select_rd_pu_device(p(folded[k]), p(rd_merge), mask, P, p(d_min), p(d_max), stream=st)
        torch.cuda.synchronize()
        maps[k] = (d_min.cpu().numpy().copy(), d_max.cpu().numpy().copy())
    valid = h_cand["cost_rd"] != 0xFFFFFFFF
    wins = h_plain["nxn"]["part"][:, 21:] == capi.RD_PART_INTRA_NXN
    kept = h_folded["nxn"]["part"][:, 21:] == capi.RD_PART_INTRA_NXN
    per_picture = lambda m: m.reshape(P, -1).sum(axis=1)
    choice = {"nodes_8x8_per_picture": n * 64, "nxn_valid_per_picture_mean": float(per_picture(valid).mean()),
              "nxn_wins_per_picture": {"mean": float(per_picture(wins).mean()), "min": int(per_picture(wins).min()), "max": int(per_picture(wins).max())},
              "nxn_survives_the_fold_per_picture": {"mean": float(per_picture(kept).mean()), "min": int(per_picture(kept).min()), "max": int(per_picture(kept).max())},
              "intra_2nx2n_survives_the_fold_at_level_3_per_picture_without_the_candidate": float(per_picture(h_folded["three"]["part"][:, 21:] == capi.RD_PART_INTRA).mean()),
              "both_folds_into": "the inter records folded at tu_depths 3",
              "depth_maps_with_the_candidate_against_without": {
                  "entries_of_depth_min_changed": int((maps["nxn"][0] != maps["three"][0]).sum()), "entries_of_depth_max_changed": int((maps["nxn"][1] != maps["three"][1]).sum()),
                  "entries": int(maps["nxn"][1].size), "mean_depth_max_with": float(maps["nxn"][1].mean()), "mean_depth_max_without": float(maps["three"][1].mean())}}
    print("choice:", json.dumps(choice), flush=True)

    runs = {
        "nxn": lambda: stage("nxn", plain["nxn"], x=cand),
        "nxn_fold": lambda: stage("nxn", folded["nxn"], p(folded["nxn"]), p(rd_merge), mask, x=cand_f),
        "three": lambda: stage("three", plain["three"]),
        "first4": first_pass_4x4,
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
    where = {"nxn": plain["nxn"], "nxn_fold": folded["nxn"], "three": plain["three"], "first4": first4}
    sha = {name: hashlib.sha256(where[name].cpu().numpy().tobytes()).hexdigest() for name in runs}

    out = {"tool": "tools/intra_rd_nxn_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pictures_priced": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8", "max_range": R},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the runs; ms = median of the windows",
           "device_equals_host_form_on_picture_1": bool(equal), "what_the_candidate_changes": choice, "quality_bd_rate": "not measured",
           "added_work_by_a_count_of_the_code_without_against_with_the_candidate": ADDED_WORK, "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": args.launches, "sha256": sha[name]}
        print(f"{name:8s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  sha256 {sha[name][:16]}", flush=True)

    def ratio(num, den):
        per_round = [sum(ms[x][r] for x in num) / ms[den][r] for r in range(args.repeats)]
        return {"ratio_of_medians": sum(statistics.median(ms[x]) for x in num) / statistics.median(ms[den]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["against_the_stage_without_the_candidate"] = {"a_over_c": ratio(["nxn"], "three"), "b_over_c": ratio(["nxn_fold"], "three"),
                                                      "a_plus_d_over_c": ratio(["nxn", "first4"], "three")}
    print("against three depths:", json.dumps(out["against_the_stage_without_the_candidate"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
