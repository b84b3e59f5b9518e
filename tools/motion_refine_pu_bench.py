#!/usr/bin/env python3
"""Measurement: the quarter-sample refinement of the PUs beside the refinement of the square nodes the library had before, on the bench GOP's
geometry (64 pictures of 1920 x 1080, int16 planes at 8 bit resident in HBM: 63 picture pairs = 32 130 CTUs per launch).

Per launch, at vectors of search range 8 (the inputs are what the three searches wrote for the same pictures), HIP events on the caller's stream
around:
  (a) fhevc_motion_refine_device                          the 85 square nodes (the baseline: same arithmetic, four tile passes per CTU)
  (b) fhevc_motion_refine_pu_device, the 124 only         fourteen tile passes
  (c) fhevc_motion_refine_pu_device, the 384 only         twelve tile passes, four 4x4 Hadamards each
  (d) fhevc_motion_refine_pu_device, both families        twenty-six tile passes
  (e) both PU searches and (d) on one stream              what a caller pays for all 508 quarter-sample PU costs of a CTU
All run in ONE process on one device, INTERLEAVED: a round times a .. e one after the other, --repeats rounds; every figure is the median over the
rounds with the smallest and largest next to it, and the spread is (largest - smallest) / median.
No time is required.  The expectation from a count of the code is d / a about 26 / 4 = six to seven; the measured ratio is recorded next to it.

Needs an MI355X; without one it fails.  Writes profiles/motion_refine_pu.json (--out)."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fasthevc_amd import capi, frames  # noqa: E402


def _commit(given):
    if given:
        return given
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--range", type=int, default=8, help="search range of the inputs = max_range of the refinements")
    ap.add_argument("--repeats", type=int, default=7, help="interleaved rounds (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=2, help="launches per timed window")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_refine_pu.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_refine_pu_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, r = args.width, args.height, args.frames, args.qp, args.range
    ys = [y.astype(np.int16) for y in frames.pan_clip(W, H, NF)]
    flat, org, stride, fs = frames.guarded_plane(ys, 8, np.int16, margin=80, poison=None)
    planes = torch.from_numpy(flat).cuda()
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (planes.data_ptr() + 2 * org, 2, stride, fs, NF)

    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = (NF - 1) * ctx.num_ctus
    buf = lambda per: torch.zeros(n * per * 16, dtype=torch.uint8, device="cuda")
    d_nodes, d_pus, d_small = buf(85), buf(capi.PUS_PER_CTU), buf(capi.PUS_SMALL_PER_CTU)
    q_nodes, q_pus, q_small = buf(85), buf(capi.PUS_PER_CTU), buf(capi.PUS_SMALL_PER_CTU)
    # the inputs: the three searches' own output for these pictures
    ctx.motion_search_device(*layout, d_nodes.data_ptr(), stream=st, qp=qp, search_range=r)
    ctx.motion_search_pu_device(*layout, d_pus.data_ptr(), None, stream=st, qp=qp, search_range=r)
    ctx.motion_search_pu_small_device(*layout, d_small.data_ptr(), stream=st, qp=qp, search_range=r)
    torch.cuda.synchronize()

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.launches

    def figure(ev):
        med = statistics.median(ev)
        return {"ms": med, "ms_min": min(ev), "ms_max": max(ev), "spread": (max(ev) - min(ev)) / med, "windows": len(ev), "launches_per_window": args.launches}

    def refine_pu(pus, small):
        ctx.motion_refine_pu_device(*layout, d_pus.data_ptr() if pus else None, q_pus.data_ptr() if pus else None, d_small.data_ptr() if small else None,
                                    q_small.data_ptr() if small else None, stream=st, qp=qp, max_range=r)

    def search_then_refine():
        ctx.motion_search_pu_device(*layout, d_pus.data_ptr(), None, stream=st, qp=qp, search_range=r)
        ctx.motion_search_pu_small_device(*layout, d_small.data_ptr(), stream=st, qp=qp, search_range=r)
        refine_pu(True, True)

    runs = {
        "a_refine_square_nodes": lambda: ctx.motion_refine_device(*layout, d_nodes.data_ptr(), q_nodes.data_ptr(), stream=st, qp=qp, max_range=r),
        "b_refine_pus_124": lambda: refine_pu(True, False),
        "c_refine_pus_small_384": lambda: refine_pu(False, True),
        "d_refine_pus_508": lambda: refine_pu(True, True),
        "e_search_and_refine_pus_508": search_then_refine,
    }
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, fn in runs.items():
            ev[k].append(window(fn))
    res = {k: figure(v) for k, v in ev.items()}
    a, b, c, d, e = (res[k]["ms"] for k in runs)
    out = {"tool": "tools/motion_refine_pu_bench.py", "commit": _commit(args.commit), "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "picture_pairs": NF - 1, "ctus_per_launch": n, "qp": qp, "range": r, "planes": "int16", "bit_depth": 8,
                        "clip": "frames.pan_clip", "inputs": "the searches' own vectors (SATD mode)"},
           "timing": "per launch; HIP events on the caller's stream around a window of launches ending in a synchronise; a .. e interleaved round by round in "
                     "one process, each warmed by one launch; ms = median over the rounds; spread = (max - min) / median",
           "baseline": "(a) fhevc_motion_refine_device: same results as the parent commit's kernel (its tile prediction moved into a shared header)",
           "expectation": "d / a about 26 / 4 tile passes = six to seven; recorded, not required",
           "runs": res,
           "checks": {"b_over_a": b / a, "c_over_a": c / a, "d_over_a": d / a, "d_over_b_plus_c": d / (b + c), "e_minus_d_ms": e - d,
                      "largest_spread": max(v["spread"] for v in res.values())}}
    for k, v in res.items():
        print(f"{k:30s}: {v['ms']:.3f} ms  (min {v['ms_min']:.3f}, max {v['ms_max']:.3f})", flush=True)
    print(f"b/a {b / a:.2f}  c/a {c / a:.2f}  d/a {d / a:.2f}  (expected about 6.5)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
