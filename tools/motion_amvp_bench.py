#!/usr/bin/env python3
"""Measurement: the re-pricing of refined costs against neighbour predictors (fhevc_motion_amvp_device, k_motion_amvp.hip) on the bench GOP's geometry.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 P pictures = 32 130 CTUs per call.  The inputs are real: the SAD searches of
all three families at --range (default 64: HM's SearchRange) and their quarter-sample refinement run once, the stage reads that output.  The protocol is
tools/pu_shape_bench.py's: the legs are timed in ONE process, interleaved (every round times each of them once), each as a window of warmed, repeated
launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows with the smallest and
largest next to it:
  a   the stage on all three families (reads 9 488 B of records per CTU, writes 9 488 B)
  b   the stage on the nodes alone (reads and writes 1 360 B)
  c   a device-to-device hipMemcpyAsync of the 9 488 input bytes per CTU: it moves what (a) moves, 9 488 B read and 9 488 B written
  d   the PU launch of fhevc_motion_refine_pu_wide_device that the stage follows (both PU families, no nodes)
  e0  fhevc_pu_shape_select_merge_device on the refinement's records;  e1  the same on the re-priced records
Recorded: a / c and a / d with the run-to-run spread, and on which side of the expectation (a near c: the kernel is bound by memory) the kernel fell; no
threshold is fixed.  Also, on the first --stat-pictures pictures of the clip: the mean vector bits before (against zero) and after (against the chosen
predictor), the share of priced entries whose cost falls, how often a PU's merge cost is the smaller one before and after, and how often the
selection's best partition size changes.  Before anything is timed the device output of one picture is compared with the host twin.

Needs an MI355X; without one it fails.  Writes profiles/motion_amvp.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fasthevc_amd import capi, frames  # noqa: E402

HBM_PEAK = 8.0e12
PER = (85, 124, 384)
IN_BYTES = sum(PER) * 16       # 9 488 per CTU
MARK = 0xFFFFFFFF


def eg_bits(v):
    """xGetExpGolombNumberOfBits at cost scale 0, on an int64 array"""
    t = np.where(v <= 0, (-v << 1) + 1, v << 1)
    return 2 * np.floor(np.log2(t)).astype(np.int64) + 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--range", type=int, default=64, help="search range of the searches and max_range of the refinement (1..64)")
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=50, help="launches per window of the stage, the copy and the selection (the refinement: two)")
    ap.add_argument("--stat-pictures", type=int, default=8, help="pictures whose records are brought to the host for the statistics")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_amvp.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_amvp_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, R = args.width, args.height, args.frames, args.qp, args.range
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    total = P * n
    d8 = torch.from_numpy(np.stack(frames.pan_clip(W, H, NF))).cuda()
    found = [torch.zeros((total, k, 16), dtype=torch.uint8, device="cuda") for k in PER]
    # each set of 593 entries per CTU in ONE allocation, so that the yardstick is one copy of exactly the bytes the stage reads
    offs = np.cumsum([0] + [total * k * 16 for k in PER])

    def entries():
        t = torch.zeros((total * IN_BYTES,), dtype=torch.uint8, device="cuda")
        ptrs = [t.data_ptr() + int(o) for o in offs[:3]]
        assert all(p % 16 == 0 for p in ptrs)
        return t, ptrs

    refined_all, refined = entries()
    priced_all, priced = entries()
    copy_dst = torch.zeros_like(refined_all)
    mvp = [torch.zeros((total, k, 8), dtype=torch.uint8, device="cuda") for k in PER]
    merge = [torch.zeros((total, k, 16), dtype=torch.uint8, device="cuda") for k in PER[1:]]
    shapes = [torch.zeros((total, 85, 16), dtype=torch.uint8, device="cuda") for _ in range(2)]
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)

    ctx.motion_search_pu_wide_device(*layout, found[0].data_ptr(), found[1].data_ptr(), found[2].data_ptr(), stream=st, qp=qp, search_range=R)
    ctx.motion_refine_pu_wide_device(*layout, found[0].data_ptr(), refined[0], found[1].data_ptr(), refined[1], found[2].data_ptr(), refined[2],
                                     stream=st, qp=qp, max_range=R)
    ctx.motion_merge_pu_device(*layout, refined[0], merge[0].data_ptr(), merge[1].data_ptr(), stream=st, qp=qp, max_range=R)
    ctx.motion_amvp_device(NF, *refined, *priced, *[m.data_ptr() for m in mvp], stream=st, qp=qp)
    torch.cuda.synchronize()

    def stage_all():
        ctx.motion_amvp_device(NF, *refined, *priced, stream=st, qp=qp)

    def stage_nodes():
        ctx.motion_amvp_device(NF, refined[0], None, None, priced[0], stream=st, qp=qp)

    def copy_inputs():
        copy_dst.copy_(refined_all, non_blocking=True)      # hipMemcpyAsync, device to device, on the current stream

    def refine_pus():
        ctx.motion_refine_pu_wide_device(*layout, None, None, found[1].data_ptr(), refined[1], found[2].data_ptr(), refined[2], stream=st, qp=qp, max_range=R)

    def select_plain():
        ctx.pu_shape_select_merge_device(*refined, merge[0].data_ptr(), merge[1].data_ptr(), P, shapes[0].data_ptr(), stream=st)

    def select_priced():
        ctx.pu_shape_select_merge_device(*priced, merge[0].data_ptr(), merge[1].data_ptr(), P, shapes[1].data_ptr(), stream=st)

    # the result first: picture 0 against the host twin; then the statistics on the first pictures
    sp = min(args.stat_pictures, P)

    def host(t_all, k_index, pictures, dtype=capi.MOTION_QPEL_DTYPE):
        o, k = int(offs[k_index]), PER[k_index]
        return t_all[o:o + pictures * n * k * 16].cpu().numpy().view(dtype).reshape(pictures, n, k)

    before = [host(refined_all, i, sp) for i in range(3)]
    after = [host(priced_all, i, sp) for i in range(3)]
    preds = [m[:sp * n].cpu().numpy().reshape(-1).view(capi.MOTION_MVP_DTYPE).reshape(sp, n, k) for m, k in zip(mvp, PER)]
    twin = capi.motion_amvp_picture(before[0][0], before[1][0], before[2][0], W, H, qp=qp, with_mvp=True)
    equal = all(twin[i].tobytes() == after[i][0].tobytes() and twin[3 + i].tobytes() == preds[i][0].tobytes() for i in range(3))
    print("device equals the host twin on picture 0:", equal, flush=True)
    select_plain()
    select_priced()
    torch.cuda.synchronize()
    stats = {"pictures": sp, "families": {}}
    for name, b, a, m in zip(("nodes", "pus", "pus_small"), before, after, preds):
        ok = m["idx"] != 255
        bits0 = eg_bits(b["mvx"][ok].astype(np.int64)) + eg_bits(b["mvy"][ok].astype(np.int64))
        stats["families"][name] = {"priced_entries": int(ok.sum()), "mean_vector_bits_against_zero": float(bits0.mean()),
                                   "mean_vector_bits_against_the_predictor": float(m["bits"][ok].mean()),
                                   "share_of_entries_whose_cost_falls": float((a["cost_best"][ok] < b["cost_best"][ok]).mean()),
                                   "share_of_entries_whose_cost_rises": float((a["cost_best"][ok] > b["cost_best"][ok]).mean()),
                                   "share_priced_against_a_filled_zero": float((m["src"][ok] == 5).mean())}
    mrg = [x[:sp * n].cpu().numpy().reshape(-1).view(capi.MOTION_MERGE_DTYPE).reshape(sp, n, k) for x, k in zip(merge, PER[1:])]
    both = [(g["cost_best"] != MARK) & (b["cost_best"] != MARK) for g, b in zip(mrg, before[1:])]
    count = sum(int(x.sum()) for x in both)
    stats["merge_cost_is_the_smaller_one"] = {
        "pu_entries_with_both_costs": count,
        "share_before": sum(int((g["cost_best"][x] < b["cost_best"][x]).sum()) for g, b, x in zip(mrg, before[1:], both)) / count,
        "share_after": sum(int((g["cost_best"][x] < a["cost_best"][x]).sum()) for g, a, x in zip(mrg, after[1:], both)) / count}
    s0, s1 = (s[:sp * n].cpu().numpy().reshape(-1).view(capi.SHAPE_DTYPE).reshape(sp, n, 85) for s in shapes)
    valid = s0["best"] != 255
    stats["selection"] = {"valid_nodes": int(valid.sum()), "share_whose_best_changes": float((s0["best"][valid] != s1["best"][valid]).mean()),
                          "share_2Nx2N_before": float((s0["best"][valid] == 0).mean()), "share_2Nx2N_after": float((s1["best"][valid] == 0).mean())}
    print("statistics:", json.dumps(stats), flush=True)

    runs = {"a_stage_all_families": (stage_all, args.launches), "b_stage_nodes": (stage_nodes, args.launches), "c_copy_of_the_inputs": (copy_inputs, args.launches),
            "d_refine_pus": (refine_pus, 2), "e0_select_merge_on_refined": (select_plain, args.launches), "e1_select_merge_on_repriced": (select_priced, args.launches)}

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    for fn, _ in runs.values():      # warm-up: every shape the timed windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(args.repeats):     # interleaved: one window of each per round
        for name, (fn, launches) in runs.items():
            ms[name].append(window(fn, launches))

    moved = {"a_stage_all_families": 2 * IN_BYTES, "b_stage_nodes": 2 * 85 * 16, "c_copy_of_the_inputs": 2 * IN_BYTES}
    out = {"tool": "tools/motion_amvp_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "p_pictures": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "range": R, "planes": "uint8",
                        "record_bytes_per_ctu": IN_BYTES},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the legs; ms = median of the windows",
           "device_equals_host_twin_on_picture_0": bool(equal), "statistics": stats, "runs": {}}
    for name, (fn, launches) in runs.items():
        v = ms[name]
        r = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v), "launches_per_window": launches}
        if name in moved:
            nbytes = total * moved[name]
            r.update(bytes_from_shapes=nbytes, bytes_per_ctu=moved[name], tb_per_s=nbytes / (r["ms"] * 1e-3) / 1e12,
                     share_of_8_tb_per_s_hbm_peak=nbytes / (r["ms"] * 1e-3) / HBM_PEAK)
        out["runs"][name] = r
        print(f"{name:28s}: {r['ms'] * 1e3:10.1f} us  ({r['ms_min'] * 1e3:.1f} .. {r['ms_max'] * 1e3:.1f})" +
              (f"  {r['tb_per_s']:.2f} TB/s from shapes" if "tb_per_s" in r else ""), flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios"] = {"a_over_c": ratio("a_stage_all_families", "c_copy_of_the_inputs"), "a_over_d": ratio("a_stage_all_families", "d_refine_pus"),
                     "e1_over_e0": ratio("e1_select_merge_on_repriced", "e0_select_merge_on_refined")}
    ac = out["ratios"]["a_over_c"]["ratio_of_medians"]
    out["expectation"] = {"statement": "a lies near c: the stage moves the copy's bytes and is bound by memory", "a_over_c": ac,
                          "side": "faster than the copy" if ac < 1.0 else "slower than the copy"}
    print("ratios:", json.dumps(out["ratios"]), "expectation:", json.dumps(out["expectation"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
