#!/usr/bin/env python3
"""Measurement: the motion search of the PUs with a 4-sample side beside the two searches the library had before, on the bench GOP's geometry
(64 pictures of 1920 x 1080, int16 planes at 8 bit resident in HBM: 63 picture pairs = 32 130 CTUs per launch).

Per launch, at search ranges 4 and 8 and in both distortions, HIP events on the caller's stream around:
  (a) fhevc_motion_search_device             the 85 square nodes (untouched by this tool's commit: the baseline)
  (b) fhevc_motion_search_pu_device          the 124 PUs whose sides are multiples of 8, alone (untouched as well)
  (c) fhevc_motion_search_pu_small_device    the 384 PUs with a 4-sample side: the new kernel
All three run in ONE process on one device, INTERLEAVED: a round times a, b, c one after the other, --repeats rounds; every figure is the median
over the rounds with the smallest and largest next to it, and the spread is (largest - smallest) / median.
No ratio is required.  The expectation from an instruction count (four 4x4 Hadamards: 256 add/sub + 64 abs per tile and vector against 384 + 64
of one 8x8; three quad permutes against a six-step butterfly) is c about a, and c below b; which side c falls on is recorded.

Needs an MI355X; without one it fails.  Writes profiles/motion_pu_small.json (--out)."""
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
    ap.add_argument("--repeats", type=int, default=7, help="interleaved rounds per configuration (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=2, help="launches per timed window")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_pu_small.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_pu_small_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    ys = [y.astype(np.int16) for y in frames.pan_clip(W, H, NF)]
    flat, org, stride, fs = frames.guarded_plane(ys, 8, np.int16, margin=80, poison=None)
    planes = torch.from_numpy(flat).cuda()
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (planes.data_ptr() + 2 * org, 2, stride, fs, NF)

    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = (NF - 1) * ctx.num_ctus
    d_nodes = torch.zeros(n * 85 * 16, dtype=torch.uint8, device="cuda")
    d_pus = torch.zeros(n * capi.PUS_PER_CTU * 16, dtype=torch.uint8, device="cuda")
    d_small = torch.zeros(n * capi.PUS_SMALL_PER_CTU * 16, dtype=torch.uint8, device="cuda")

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

    out = {"tool": "tools/motion_pu_small_bench.py", "commit": _commit(args.commit), "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "picture_pairs": NF - 1, "ctus_per_launch": n, "qp": qp, "planes": "int16", "bit_depth": 8,
                        "clip": "frames.pan_clip"},
           "timing": "per launch; HIP events on the caller's stream around a window of launches ending in a synchronise; a, b, c interleaved round by "
                     "round in one process, each warmed by one launch; ms = median over the rounds; spread = (max - min) / median",
           "baseline": "(a) fhevc_motion_search_device and (b) fhevc_motion_search_pu_device: kernels of the parent commit, which this tool's commit does not touch",
           "expectation": "c about a (within the measured spread or below), and c below b; recorded, not required", "runs": {}, "checks": {}}
    for sad in (False, True):
        ctx.set_motion_distortion("sad" if sad else "satd")
        for r in (4, 8):
            runs = {
                "a_square_nodes": lambda: ctx.motion_search_device(*layout, d_nodes.data_ptr(), stream=st, qp=qp, search_range=r),
                "b_pus_124": lambda: ctx.motion_search_pu_device(*layout, d_pus.data_ptr(), None, stream=st, qp=qp, search_range=r),
                "c_pus_small_384": lambda: ctx.motion_search_pu_small_device(*layout, d_small.data_ptr(), stream=st, qp=qp, search_range=r),
            }
            for fn in runs.values():
                fn()
            torch.cuda.synchronize()
            ev = {k: [] for k in runs}
            for _ in range(args.repeats):
                for k, fn in runs.items():
                    ev[k].append(window(fn))
            key = f"{'sad' if sad else 'satd'}_range{r}"
            res = {k: figure(v) for k, v in ev.items()}
            a, b, c = (res[k]["ms"] for k in runs)
            spread_ms = max(res[k]["ms_max"] - res[k]["ms_min"] for k in runs)
            out["runs"][key] = res
            out["checks"][key] = {"c_over_a": c / a, "c_over_b": c / b, "largest_spread_ms": spread_ms, "c_at_most_a_plus_spread": bool(c <= a + spread_ms),
                                  "c_below_b": bool(c < b)}
            print(f"{key:12s}: a {a:.3f} ms  b {b:.3f} ms  c {c:.3f} ms  c/a {c / a:.3f}  c/b {c / b:.3f}  spread {spread_ms:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
