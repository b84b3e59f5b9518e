#!/usr/bin/env python3
"""Measurement: the intra RD stage that searches the first pass's candidate lists (fhevc_intra_rd_search_device: the two search instances of
k_motion_rd.hip) against the one-mode stage with the NxN candidate (fhevc_intra_rd_nxn_device) on the same pictures, and the two first passes with their
list outputs.  tools/intra_rd_nxn_bench.py's protocol.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): pictures 1..63 = 32 130 CTUs per call.  The inter chain of fhevc_p_tree_rd_qt_frame
at tu_depths 3 up to the folded inter records and the merge records' RD records runs once, and so do the first passes of pictures 1..63 (records and lists
at 8 candidates).  The legs are timed in ONE process, interleaved, each as a window of warmed, repeated launches between HIP events on one explicit stream;
every figure is the median of --repeats windows with the smallest and largest next to it:
  search      fhevc_intra_rd_search_device under the default rule, with d_modes4 and d_nxn, plain
  search_fold the same with the calm gate (skip_mask 3) and the fold in place into a copy of the inter records
  search_one  the same stage at counts all 1, append_planar 0: the price of the mechanism alone (its bytes are the NxN stage's)
  nxn         fhevc_intra_rd_nxn_device on the first passes' records
  lists       fhevc_intra_first_pass_candidates_device at 8 candidates
  lists4      fhevc_intra_first_pass_4x4_device, lists only, at 8 candidates
Recorded, not asserted: the ratios with the run-to-run spread; how often the winner is not list position 0 per level, how often the second wins step B, how
often NxN wins and survives the fold; how many entries of the RD tree's depth maps change and the mean depth_max against the one-mode stage.  Before
anything is timed the device's records of picture 1 are compared with the host form.  Quality (BD-rate): not measured.

Needs an MI355X; without one it fails.  Writes profiles/intra_rd_search.json (--out)."""
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

# by a count of the code, per CTU: depth-0 positions of step A, full three-depth runs of step B, 4-point passes of the 4x4 PUs' positions
EXPECTED_WORK = {"one_mode_stage": {"three_depth_runs": 1}, "search_default_rule": {"depth0_positions": 9, "three_depth_runs": 2, "pu_positions": 9},
                 "search_counts_one": {"depth0_positions": 1, "three_depth_runs": 1, "pu_positions": 1}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest); at least 7")
    ap.add_argument("--launches", type=int, default=5, help="launches per window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_rd_search.json"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("intra_rd_search_bench.py reports medians of at least 7 windows")

    import torch
    if not torch.cuda.is_available():
        sys.exit("intra_rd_search_bench.py needs an MI355X: no GPU is visible")
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
    modes, modes4 = buf(85, 8), buf(256, 8)
    ctx.intra_first_pass_device(*current, p(first), stream=st, qp=qp)
    ctx.intra_first_pass_4x4_device(*current, p(first4), None, stream=st, qp=qp, num_candidates=0)
    lists = lambda: ctx.intra_first_pass_candidates_device(*current, p(modes), stream=st, qp=qp, num_candidates=8)
    lists4 = lambda: ctx.intra_first_pass_4x4_device(*current, None, p(modes4), stream=st, qp=qp, num_candidates=8)
    lists()
    lists4()
    torch.cuda.synchronize()
    del found, fine
    KINDS = ("nxn", "search", "one")
    ONE = capi.intra_search_rule((1, 1, 1, 1), 1, 0)
    plain = {k: buf() for k in KINDS}
    folded = {k: buf() for k in KINDS}
    cand = {k: buf(64) for k in KINDS}
    cand_f = {k: buf(64) for k in KINDS}

    def stage(kind, out, x, fold=None, m=None, k=0):
        if kind == "nxn":
            ctx.intra_rd_nxn_device(*current, p(first), p(first4), p(out), p(x), d_fold=fold, d_rd_merge=m, skip_mask=k, stream=st, qp=qp)
        else:
            ctx.intra_rd_search_device(*current, p(modes), 8, p(modes4), 8, p(out), rule=ONE if kind == "one" else None, d_nxn=p(x), d_fold=fold, d_rd_merge=m, skip_mask=k,
                                       stream=st, qp=qp)

    # the result first: picture 1 against the host form, plain and gated + folded
    for kind in KINDS:
        stage(kind, plain[kind], cand[kind])
        folded[kind].copy_(inter)
        stage(kind, folded[kind], cand_f[kind], p(folded[kind]), p(rd_merge), mask)
    torch.cuda.synchronize()
    host = lambda t, dt, per=85: t.cpu().numpy().view(dt).reshape(total, per)
    h_modes, h_modes4 = modes.cpu().numpy().reshape(total, 85, 8), modes4.cpu().numpy().reshape(total, 256, 8)
    h_inter, h_merge = host(inter, capi.MOTION_RD_PU_DTYPE), host(rd_merge, capi.MOTION_RD_DTYPE)
    h_plain = {k: host(plain[k], capi.MOTION_RD_PU_DTYPE) for k in KINDS}
    h_folded = {k: host(folded[k], capi.MOTION_RD_PU_DTYPE) for k in KINDS}
    h_cand = host(cand["search"], capi.INTRA_RD_NXN_DTYPE, 64)
    cur = pics[1].astype(np.int16)
    hp, hx = ctx.intra_rd_search(cur, h_modes[:n], h_modes4[:n], origin=0, stride=W, qp=qp, with_nxn=True)
    hf = ctx.intra_rd_search(cur, h_modes[:n], h_modes4[:n], fold=h_inter[:n], rd_merge=h_merge[:n], skip_mask=mask, origin=0, stride=W, qp=qp)
    equal = (hp.tobytes() == h_plain["search"][:n].tobytes() and hx.tobytes() == h_cand[:n].tobytes() and hf.tobytes() == h_folded["search"][:n].tobytes() and
             cand["search"].cpu().numpy().tobytes() == cand_f["search"].cpu().numpy().tobytes())
    print("device equals the host form on picture 1:", equal, flush=True)
    if not equal:
        sys.exit("the device output of picture 1 differs from the host form: nothing is timed")
    # the lists' first bytes are the first passes' winners, so counts 1 must give the one-mode stage's bytes
    one_is_nxn = plain["one"].cpu().numpy().tobytes() == plain["nxn"].cpu().numpy().tobytes() and cand["one"].cpu().numpy().tobytes() == cand["nxn"].cpu().numpy().tobytes()
    print("counts all 1 give the one-mode stage's bytes:", one_is_nxn, flush=True)

    # what the search changes, and what the tree makes of it
    d_min, d_max = (torch.zeros((total * 256,), dtype=torch.uint8, device="cuda") for _ in range(2))
    maps = {}
    for k in ("nxn", "search"):
        ctx.p_tree_select_rd_pu_device(p(folded[k]), p(rd_merge), mask, P, p(d_min), p(d_max), stream=st)
        torch.cuda.synchronize()
        maps[k] = (d_min.cpu().numpy().copy(), d_max.cpu().numpy().copy())
    rec = h_plain["search"]
    two = rec["part"] == capi.RD_PART_INTRA
    LV = {"level_0": slice(0, 1), "level_1": slice(1, 5), "level_2": slice(5, 21), "level_3": slice(21, 85)}
    COUNT = {"level_0": 3, "level_1": 3, "level_2": 3, "level_3": 8}
    # a second that won step B is known from the kernel's bytes only where it changed the mode: what differs from best-only is not observable from outside;
    # the host-side count is of winners that are not the step-A best, which needs the restatement -- recorded instead: position and planar shares
    not0 = {k: float(((rec["pad"][:, v, 1] > 0) & two[:, v]).sum() / max(1, two[:, v].sum())) for k, v in LV.items()}
    planar = {k: float(((rec["pad"][:, v, 1] == COUNT[k]) & two[:, v]).sum() / max(1, two[:, v].sum())) for k, v in LV.items()}
    # how often the second wins step B is not in the output bytes (pad[1] holds the list position, not the step-A rank): the numpy restatement prices the first
    # CTU row of picture 1 on the device's own lists, is held to the device's bytes there, and counts
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import intra_rd_search_ref as sr  # noqa: E402
    cw = (W + 63) // 64
    seen = {}   # (st is the stream)
    ep, ex = sr.plain(cur, 8, qp, h_modes[:cw], h_modes4[:cw], rows=(0, 1), stats=seen)
    if ep.tobytes() != h_plain["search"][:cw].tobytes() or ex.tobytes() != h_cand[:cw].tobytes():
        sys.exit("the restatement differs from the device on the first CTU row of picture 1: nothing is timed")
    second_wins = {"counted_by": "tests/intra_rd_search_ref.py on the first CTU row of picture 1, equal to the device's bytes there", "ctus": cw}
    for k, v in LV.items():
        ok = seen["pos"][:, v] >= 0
        second_wins[k] = {"nodes": int(ok.sum()), "second_wins": int(seen["second_won"][:, v][ok].sum())}
    second_wins["share_of_valid_nodes"] = float(sum(x["second_wins"] for x in second_wins.values() if isinstance(x, dict)) / max(1, sum(x["nodes"] for x in second_wins.values() if isinstance(x, dict))))
    print("second wins step B:", json.dumps(second_wins), flush=True)
    wins = rec["part"][:, 21:] == capi.RD_PART_INTRA_NXN
    wins1 = h_plain["nxn"]["part"][:, 21:] == capi.RD_PART_INTRA_NXN
    kept = h_folded["search"]["part"][:, 21:] == capi.RD_PART_INTRA_NXN
    kept1 = h_folded["nxn"]["part"][:, 21:] == capi.RD_PART_INTRA_NXN
    pu_first = h_modes4[:, :, 0].reshape(total, 16, 16)
    chosen = h_cand["modes"]   # [total, 64, 4]
    valid = h_cand["cost_rd"] != 0xFFFFFFFF
    firsts = np.stack([pu_first[:, 0::2, 0::2], pu_first[:, 0::2, 1::2], pu_first[:, 1::2, 0::2], pu_first[:, 1::2, 1::2]], axis=-1).reshape(total, 64, 4)
    per_picture = lambda m: float(m.reshape(P, -1).sum(axis=1).mean())
    cost = lambda r: float(r["cost_rd"][r["part"] != 255].astype(np.float64).mean())
    choice = {"winner_not_list_position_0_share_of_valid_2nx2n_records": not0, "appended_planar_wins_share": planar,
              "pu_mode_differs_from_its_first_byte_share_of_valid_nxn_pus": float((chosen != firsts)[valid].mean()),
              "second_wins_step_b": second_wins,
              "nodes_8x8_per_picture": n * 64,
              "nxn_wins_per_picture_mean": {"search": per_picture(wins), "one_mode": per_picture(wins1)},
              "nxn_survives_the_fold_per_picture_mean": {"search": per_picture(kept), "one_mode": per_picture(kept1)},
              "intra_survives_the_fold_per_picture_mean": {"search": per_picture(h_folded["search"]["part"] >= capi.RD_PART_INTRA), "one_mode": per_picture(h_folded["nxn"]["part"] >= capi.RD_PART_INTRA)},
              "mean_cost_rd_of_valid_plain_records": {"search": cost(h_plain["search"]), "one_mode": cost(h_plain["nxn"])},
              "depth_maps_with_the_search_against_the_one_mode_stage": {
                  "entries_of_depth_min_changed": int((maps["search"][0] != maps["nxn"][0]).sum()), "entries_of_depth_max_changed": int((maps["search"][1] != maps["nxn"][1]).sum()),
                  "entries": int(maps["search"][1].size), "mean_depth_max_with": float(maps["search"][1].mean()), "mean_depth_max_without": float(maps["nxn"][1].mean())}}
    print("choice:", json.dumps(choice), flush=True)

    runs = {
        "search": lambda: stage("search", plain["search"], cand["search"]),
        "search_fold": lambda: stage("search", folded["search"], cand_f["search"], p(folded["search"]), p(rd_merge), mask),
        "search_one": lambda: stage("one", plain["one"], cand["one"]),
        "nxn": lambda: stage("nxn", plain["nxn"], cand["nxn"]),
        "lists": lists,
        "lists4": lists4,
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
    where = {"search": plain["search"], "search_fold": folded["search"], "search_one": plain["one"], "nxn": plain["nxn"], "lists": modes, "lists4": modes4}
    sha = {name: hashlib.sha256(where[name].cpu().numpy().tobytes()).hexdigest() for name in runs}

    out = {"tool": "tools/intra_rd_search_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "pictures_priced": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "planes": "uint8", "max_range": R},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the runs; ms = median of the windows",
           "device_equals_host_form_on_picture_1": bool(equal), "counts_all_1_give_the_one_mode_stages_bytes": bool(one_is_nxn), "what_the_search_changes": choice, "quality_bd_rate": "not measured",
           "expected_work_by_a_count_of_the_code": EXPECTED_WORK, "runs": {}}
    for name in runs:
        v = ms[name]
        out["runs"][name] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v),
                             "launches_per_window": args.launches, "sha256": sha[name]}
        print(f"{name:12s}: {statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})  sha256 {sha[name][:16]}", flush=True)

    def ratio(num, den):
        per_round = [sum(ms[x][r] for x in num) / ms[den][r] for r in range(args.repeats)]
        return {"ratio_of_medians": sum(statistics.median(ms[x]) for x in num) / statistics.median(ms[den]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["against_the_one_mode_stage"] = {"search_over_nxn": ratio(["search"], "nxn"), "search_fold_over_nxn": ratio(["search_fold"], "nxn"),
                                         "search_one_over_nxn": ratio(["search_one"], "nxn"), "search_plus_lists_over_nxn": ratio(["search", "lists", "lists4"], "nxn")}
    print("against the one-mode stage:", json.dumps(out["against_the_one_mode_stage"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
