#!/usr/bin/env python3
"""Measurement: the partition-size selection on the device (fhevc_pu_shape_select_device, k_pu_shape.hip) on the bench GOP's geometry.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes): 63 P pictures = 32 130 CTUs per call.  The inputs are real: the SAD searches
of all three families at --range (default 64: HM's SearchRange) and their quarter-sample refinement run once, the selection reads that output.  Four
things are timed in ONE process, interleaved (every round times each of them once, so a drift of the machine meets all four alike), each as a window of
warmed, repeated launches between HIP events on one explicit stream, ending in a synchronise; every figure is the median of --repeats windows with the
smallest and largest next to it:
  a  the selection with d_costs (reads 9 488 B per CTU, writes 1 360 + 2 720 B)
  b  the selection without d_costs (writes 1 360 B)
  c  a device-to-device hipMemcpyAsync of the same 9 488 input bytes per CTU: the yardstick for a pass that must read those bytes once (the copy
     moves them twice, a read and a write)
  d  the PU launch of fhevc_motion_refine_pu_wide_device that the selection follows (both PU families, no nodes)
Recorded: a / c, b / c, b / d with the run-to-run spread (the smallest and largest ratio of windows of the same round), the bytes each pass needs
computed from shapes over its time, and whether b <= 2 c (the expectation; it does not make the tool fail).  Before anything is timed the device
output of one picture is compared with the host function.

Needs an MI355X; without one it fails.  Writes profiles/pu_shape.json (--out)."""
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
IN_BYTES = (85 + 124 + 384) * 16       # 9 488 per CTU
REC_BYTES, COST_BYTES = 85 * 16, 85 * 32


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--range", type=int, default=64, help="search range of the searches and max_range of the refinement (1..64)")
    ap.add_argument("--repeats", type=int, default=9, help="rounds: timed windows per figure (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=50, help="launches per window of the selection and the copy (the refinement: two)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pu_shape.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("pu_shape_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, R = args.width, args.height, args.frames, args.qp, args.range
    P = NF - 1
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    total = P * n
    d8 = torch.from_numpy(np.stack(frames.pan_clip(W, H, NF))).cuda()
    per = (85, 124, 384)
    found = [torch.zeros((total, k, 16), dtype=torch.uint8, device="cuda") for k in per]
    # the refined entries in ONE allocation, so that the yardstick is one copy of exactly the bytes the selection reads
    refined_all = torch.zeros((total * IN_BYTES,), dtype=torch.uint8, device="cuda")
    offs = np.cumsum([0] + [total * k * 16 for k in per])
    refined = [refined_all.data_ptr() + int(o) for o in offs[:3]]
    assert all(p % 16 == 0 for p in refined)
    copy_dst = torch.zeros_like(refined_all)
    d_shapes = torch.zeros((total, 85, 16), dtype=torch.uint8, device="cuda")
    d_costs = torch.zeros((total, 85, 8), dtype=torch.int32, device="cuda")
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)
    rule = capi.pu_shape_rule(32, 0, 1)    # a margin of an eighth, so that masks are not trivial; the kernel's work does not depend on the rule

    ctx.motion_search_pu_wide_device(*layout, found[0].data_ptr(), found[1].data_ptr(), found[2].data_ptr(), stream=st, qp=qp, search_range=R)
    ctx.motion_refine_pu_wide_device(*layout, found[0].data_ptr(), refined[0], found[1].data_ptr(), refined[1], found[2].data_ptr(), refined[2],
                                     stream=st, qp=qp, max_range=R)
    torch.cuda.synchronize()

    def select_with_costs():
        ctx.pu_shape_select_device(refined[0], refined[1], refined[2], P, d_shapes.data_ptr(), d_costs.data_ptr(), stream=st, rule=rule)

    def select_alone():
        ctx.pu_shape_select_device(refined[0], refined[1], refined[2], P, d_shapes.data_ptr(), None, stream=st, rule=rule)

    def copy_inputs():
        copy_dst.copy_(refined_all, non_blocking=True)      # hipMemcpyAsync, device to device, on the current stream

    def refine_pus():
        ctx.motion_refine_pu_wide_device(*layout, None, None, found[1].data_ptr(), refined[1], found[2].data_ptr(), refined[2], stream=st, qp=qp, max_range=R)

    # the result first: picture 0 against the host function
    select_with_costs()
    torch.cuda.synchronize()
    host_in = [refined_all[int(o):int(o) + n * k * 16].cpu().numpy().view(capi.MOTION_QPEL_DTYPE).reshape(n, k) for o, k in zip(offs[:3], per)]
    hrec, hcosts = capi.pu_shape_select(*host_in, W, H, rule, with_costs=True)
    grec = d_shapes[:n].cpu().numpy().reshape(-1).view(capi.SHAPE_DTYPE).reshape(n, 85)
    equal = grec.tobytes() == hrec.tobytes() and np.array_equal(d_costs[:n].cpu().numpy().view(np.uint32).reshape(n, 85, 8), hcosts)
    sizes, counts = np.unique(hrec["best"], return_counts=True)
    print("device equals the host function on picture 0:", equal, " best sizes:", dict(zip(sizes.tolist(), counts.tolist())), flush=True)

    runs = {"a_select_with_costs": (select_with_costs, args.launches), "b_select": (select_alone, args.launches),
            "c_copy_of_the_inputs": (copy_inputs, args.launches), "d_refine_pus": (refine_pus, 2)}

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

    moved = {"a_select_with_costs": IN_BYTES + REC_BYTES + COST_BYTES, "b_select": IN_BYTES + REC_BYTES, "c_copy_of_the_inputs": 2 * IN_BYTES}
    out = {"tool": "tools/pu_shape_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "p_pictures": P, "ctus_per_picture": n, "ctus": total, "qp": qp, "range": R, "planes": "uint8",
                        "input_bytes_per_ctu": IN_BYTES},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; rounds interleave the four runs; ms = median of the windows",
           "device_equals_host_function_on_picture_0": bool(equal), "runs": {}}
    for name, (fn, launches) in runs.items():
        v = ms[name]
        r = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v), "windows": len(v), "launches_per_window": launches}
        if name in moved:
            nbytes = total * moved[name]
            r.update(bytes_from_shapes=nbytes, bytes_per_ctu=moved[name], tb_per_s=nbytes / (r["ms"] * 1e-3) / 1e12,
                     share_of_8_tb_per_s_hbm_peak=nbytes / (r["ms"] * 1e-3) / HBM_PEAK)
        out["runs"][name] = r
        print(f"{name:22s}: {r['ms'] * 1e3:10.1f} us  ({r['ms_min'] * 1e3:.1f} .. {r['ms_max'] * 1e3:.1f})" +
              (f"  {r['tb_per_s']:.2f} TB/s from shapes" if "tb_per_s" in r else ""), flush=True)

    def ratio(x, y):
        per_round = [a / b for a, b in zip(ms[x], ms[y])]
        return {"ratio_of_medians": statistics.median(ms[x]) / statistics.median(ms[y]), "per_round_min": min(per_round), "per_round_max": max(per_round)}

    out["ratios"] = {"a_over_c": ratio("a_select_with_costs", "c_copy_of_the_inputs"), "b_over_c": ratio("b_select", "c_copy_of_the_inputs"),
                     "b_over_d": ratio("b_select", "d_refine_pus")}
    out["checks"] = {"b_at_most_2c": out["ratios"]["b_over_c"]["ratio_of_medians"] <= 2.0}
    print("ratios:", json.dumps(out["ratios"]), "checks:", json.dumps(out["checks"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
