#!/usr/bin/env python3
"""Measurement: the intra stage of P pictures (fhevc_intra_p_device, k_intra_p.hip) and the tree that takes its costs (fhevc_p_tree_select_intra_device) on
the bench GOP's geometry.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 P pictures = 32 130 CTUs per call.  The inputs are real: the two intra first
passes of the 63 current pictures, and for the trees the chain in front of them (SAD searches of all three families at --range, their quarter-sample
refinement, the re-pricing, the merge stages per node and per PU, the merge-aware selection, the zero-residual stage), each run once.  The protocol is
tools/motion_amvp_bench.py's: the legs are timed in ONE process, interleaved (every round times each of them once), each as a window of warmed, repeated
launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows with the smallest and largest
next to it:
  a   the intra stage with the 4x4 records (reads 5 456 B of records per CTU, writes 1 360 B)
  b   the intra stage without them (reads and writes 1 360 B)
  c   a device-to-device hipMemcpyAsync of the same bytes: 5 456 B per CTU copied, then 1 360 B per CTU copied -- what (a) reads and what it writes
  d   the two first-pass launches the stage follows (fhevc_intra_first_pass_device, fhevc_intra_first_pass_4x4_device)
  e   fhevc_p_tree_select_skip_device, maps and records
  f   fhevc_p_tree_select_intra_device on the same records and the intra stage's
Recorded: a / c and f / e with the run-to-run spread, and on which side of the expectations (a near c; f within a few microseconds of e) the kernels fell;
no threshold is fixed.  Also, on the first --stat-pictures pictures: how often intra is the own cost per level, and how often the calm gate withholds a
smaller intra cost.  Before anything is timed the device output of one picture is compared with the host twins.

Needs an MI355X; without one it fails.  Writes profiles/intra_p.json (--out)."""
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
IN_BYTES, OUT_BYTES = (85 + 256) * 16, 85 * 16       # 5 456 and 1 360 per CTU
MARK = 0xFFFFFFFF
LEVEL = np.array([0] + [1] * 4 + [2] * 16 + [3] * 64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--range", type=int, default=8, help="search range of the chain in front of the trees (1..64); it shapes the statistics, not the timed legs")
    ap.add_argument("--skip-mask", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7, help="rounds: timed windows per figure (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=50, help="launches per window (the first passes: two)")
    ap.add_argument("--stat-pictures", type=int, default=8, help="pictures whose records are brought to the host for the statistics")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_p.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("intra_p_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, R, mask = args.width, args.height, args.frames, args.qp, args.range, args.skip_mask
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    total = P * n
    d8 = torch.from_numpy(np.stack(frames.pan_clip(W, H, NF))).cuda()

    def records(per, item=16):
        return torch.zeros((total * per * item,), dtype=torch.uint8, device="cuda")

    # the stage's input in ONE allocation (the 85, behind them the 256), so that the yardstick copies exactly the bytes the stage reads
    first_all = records(85 + 256)
    first, first4 = first_all.data_ptr(), first_all.data_ptr() + total * 85 * 16
    intra, intra_no4 = records(85), records(85)
    copy_in, copy_out = torch.zeros_like(first_all), torch.zeros_like(intra)
    found, refined, priced = ([records(k) for k in PER] for _ in range(3))
    merge, merge_pu, merge_small, shapes, skip = records(85), records(124), records(384), records(85), records(85)
    maps = [[torch.zeros((total * 256,), dtype=torch.uint8, device="cuda") for _ in range(2)] for _ in range(2)]
    trees = [records(85) for _ in range(2)]
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)
    current = (d8.data_ptr() + W * H, 1, W, W * H, P)      # the P pictures themselves: what the first passes read
    ptr = lambda ts_: [t.data_ptr() for t in ts_]

    def first_passes():
        ctx.intra_first_pass_device(*current, first, stream=st, qp=qp)
        ctx.intra_first_pass_4x4_device(*current, first4, None, stream=st, qp=qp)

    first_passes()
    ctx.motion_search_pu_wide_device(*layout, *ptr(found), stream=st, qp=qp, search_range=R)
    ctx.motion_refine_pu_wide_device(*layout, found[0].data_ptr(), refined[0].data_ptr(), found[1].data_ptr(), refined[1].data_ptr(), found[2].data_ptr(),
                                     refined[2].data_ptr(), stream=st, qp=qp, max_range=R)
    ctx.motion_amvp_device(NF, *ptr(refined), *ptr(priced), stream=st, qp=qp)
    ctx.motion_merge_device(*layout, priced[0].data_ptr(), merge.data_ptr(), stream=st, qp=qp, max_range=R)
    ctx.motion_merge_pu_device(*layout, priced[0].data_ptr(), merge_pu.data_ptr(), merge_small.data_ptr(), stream=st, qp=qp, max_range=R)
    ctx.pu_shape_select_merge_device(*ptr(priced), merge_pu.data_ptr(), merge_small.data_ptr(), P, shapes.data_ptr(), stream=st)
    ctx.motion_skip_device(*layout, merge.data_ptr(), skip.data_ptr(), stream=st, qp=qp, max_range=R)
    torch.cuda.synchronize()

    def stage_with_4x4():
        ctx.intra_p_device(P, first, first4, intra.data_ptr(), stream=st, qp=qp)

    def stage_without_4x4():
        ctx.intra_p_device(P, first, None, intra_no4.data_ptr(), stream=st, qp=qp)

    def copy_same_bytes():
        copy_in.copy_(first_all, non_blocking=True)      # hipMemcpyAsync, device to device, on the current stream
        copy_out.copy_(intra, non_blocking=True)

    def tree_skip():
        ctx.p_tree_select_skip_device(shapes.data_ptr(), merge.data_ptr(), skip.data_ptr(), mask, P, maps[0][0].data_ptr(), maps[0][1].data_ptr(), trees[0].data_ptr(),
                                      stream=st)

    def tree_intra():
        ctx.p_tree_select_intra_device(shapes.data_ptr(), merge.data_ptr(), skip.data_ptr(), mask, intra.data_ptr(), P, maps[1][0].data_ptr(), maps[1][1].data_ptr(),
                                       trees[1].data_ptr(), stream=st)

    # the result first: picture 0 against the host twins; then the statistics on the first pictures
    stage_with_4x4()
    stage_without_4x4()
    tree_skip()
    tree_intra()
    torch.cuda.synchronize()
    sp = min(args.stat_pictures, P)

    def host(t, per, dtype, offset=0):
        return t[offset:offset + sp * n * per * 16].cpu().numpy().view(dtype).reshape(sp, n, per)

    h_first, h_first4 = host(first_all, 85, capi.NODE_DTYPE), host(first_all, 256, capi.NODE_DTYPE, total * 85 * 16)
    h_intra, h_no4 = host(intra, 85, capi.INTRA_P_DTYPE), host(intra_no4, 85, capi.INTRA_P_DTYPE)
    h_shapes, h_merge, h_skip = host(shapes, 85, capi.SHAPE_DTYPE), host(merge, 85, capi.MOTION_MERGE_DTYPE), host(skip, 85, capi.MOTION_SKIP_DTYPE)
    h_tree = host(trees[1], 85, capi.TREE_DTYPE)
    twin = capi.intra_p_picture(h_first[0], h_first4[0], W, H, qp=qp)
    twin_no4 = capi.intra_p_picture(h_first[0], None, W, H, qp=qp)
    t_min, t_max, t_rec = capi.p_tree_select_intra(h_shapes[0], h_merge[0], h_skip[0], mask, h_intra[0], W, H, with_tree=True)
    equal = (twin.tobytes() == h_intra[0].tobytes() and twin_no4.tobytes() == h_no4[0].tobytes() and t_rec.tobytes() == h_tree[0].tobytes() and
             t_min.tobytes() == maps[1][0][:n * 256].cpu().numpy().tobytes() and t_max.tobytes() == maps[1][1][:n * 256].cpu().numpy().tobytes())
    print("device equals the host twins on picture 0:", equal, flush=True)
    coded = (h_tree["flags"] & 12) == 0
    inside = coded & (h_intra["cost_best"] != MARK)
    taken = (h_tree["pad"][..., 0] & 1) != 0
    inter = np.minimum(h_shapes["cost_best"], h_merge["cost_best"])
    calm = (h_merge["cost_best"] < h_shapes["cost_best"]) & ((h_skip["flags"] & mask) != 0)
    withheld = coded & calm & (h_intra["cost_best"] < inter)
    stats = {"pictures": sp, "skip_mask": mask, "share_of_8x8_intra_records_that_are_NxN": float((h_intra["part"][..., 21:][inside[..., 21:]] == 1).mean()), "levels": {}}
    for lvl in range(4):
        sel = LEVEL == lvl
        c = int(coded[..., sel].sum())
        stats["levels"][str(lvl)] = {"coded_nodes": c, "share_whose_own_cost_is_intra": float(taken[..., sel].sum() / max(c, 1)),
                                     "share_calm": float((coded & calm)[..., sel].sum() / max(c, 1)),
                                     "share_where_the_gate_withholds_a_smaller_intra_cost": float(withheld[..., sel].sum() / max(c, 1))}
    print("statistics:", json.dumps(stats), flush=True)

    runs = {"a_stage_with_4x4": (stage_with_4x4, args.launches), "b_stage_without_4x4": (stage_without_4x4, args.launches),
            "c_copy_of_the_same_bytes": (copy_same_bytes, args.launches), "d_two_first_passes": (first_passes, 2), "e_tree_skip": (tree_skip, args.launches),
            "f_tree_intra": (tree_intra, args.launches)}

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

    moved = {"a_stage_with_4x4": IN_BYTES + OUT_BYTES, "b_stage_without_4x4": 2 * OUT_BYTES, "c_copy_of_the_same_bytes": 2 * (IN_BYTES + OUT_BYTES),
             "e_tree_skip": 2 * OUT_BYTES + 85 + OUT_BYTES + 512, "f_tree_intra": 3 * OUT_BYTES + 85 + 64 + OUT_BYTES + 512}
    out = {"tool": "tools/intra_p_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "p_pictures": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "range": R, "planes": "uint8",
                        "stage_bytes_in_per_ctu": IN_BYTES, "stage_bytes_out_per_ctu": OUT_BYTES},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the legs; ms = median of the windows",
           "note": "the copy leg reads AND writes every byte the stage only reads or only writes: bytes_from_shapes counts both directions of both copies",
           "device_equals_host_twins_on_picture_0": bool(equal), "statistics": stats, "runs": {}}
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

    out["ratios"] = {"a_over_c": ratio("a_stage_with_4x4", "c_copy_of_the_same_bytes"), "b_over_a": ratio("b_stage_without_4x4", "a_stage_with_4x4"),
                     "a_over_d": ratio("a_stage_with_4x4", "d_two_first_passes"), "f_over_e": ratio("f_tree_intra", "e_tree_skip")}
    ac, fe = out["ratios"]["a_over_c"]["ratio_of_medians"], out["ratios"]["f_over_e"]["ratio_of_medians"]
    out["expectation"] = {"statement": "a lies near c (the stage moves the copy's bytes once); f lies within a few microseconds of e", "a_over_c": ac,
                          "a_side": "faster than the copy" if ac < 1.0 else "slower than the copy", "f_over_e": fe,
                          "f_minus_e_us": (statistics.median(ms["f_tree_intra"]) - statistics.median(ms["e_tree_skip"])) * 1e3}
    print("ratios:", json.dumps(out["ratios"]), "expectation:", json.dumps(out["expectation"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
