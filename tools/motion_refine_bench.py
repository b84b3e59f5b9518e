#!/usr/bin/env python3
"""Measurement: the quarter-sample motion refinement beside the integer search on the bench GOP's geometry (64 pictures of 1920 x 1080, int16 planes
resident in HBM: 63 picture pairs = 32 130 CTUs per launch).

Per launch: HIP events on the caller's stream around a window of warmed launches that ends in a synchronise; every figure is the median of
--repeats windows with the smallest and largest next to it.  Measured in ONE process on one device:
  * the refinement alone (fhevc_motion_refine_device) on the nodes of the +-8 SATD search, and on those of the +-4 search;
  * the +-4 and the +-8 SATD searches alone (fhevc_motion_search_device);
  * search plus refinement queued on one stream, for both ranges;
  * the refinement at max_range 64 (the MR = 64 layout) on the nodes of the +-64 SAD search (fhevc_motion_search_pu_wide_device).
One statement is recorded (it does not make the tool fail): the refinement takes less time than the +-8 search.  A count from the code gives
4 levels x 64 tiles x 18 candidates = 4 608 tile Hadamards per CTU against 5 184 (+-4) and 18 496 (+-8) of the search, plus about 1 500 filter
multiply-adds per tile candidate.

Every leg's figures carry the SHA-256 of the buffers it wrote: the inputs are seeded, so two builds that behave alike give equal digests.  --lib times
another build of the library (A/B of a kernel variant) under the same protocol.

Needs an MI355X; without one it fails.  Writes profiles/motion_refine.json (--out)."""
import argparse
import hashlib
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
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per figure (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=3, help="launches per window")
    ap.add_argument("--lib", default=None, help="another build of the library to measure (default: the tree's own)")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_refine.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_refine_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    ys = [y.astype(np.int16) for y in frames.pan_clip(W, H, NF)]
    flat, org, stride, fs = frames.guarded_plane(ys, 8, np.int16, margin=80, poison=None)
    planes = torch.from_numpy(flat).cuda()
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (planes.data_ptr() + 2 * org, 2, stride, fs, NF)

    def measure(fn, written):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1) / args.launches)
        sha = hashlib.sha256()
        for t in written:
            sha.update(t.cpu().numpy().tobytes())
        return {"ms": statistics.median(ev), "ms_min": min(ev), "ms_max": max(ev), "windows": args.repeats, "launches_per_window": args.launches,
                "sha256": sha.hexdigest()}

    ctx = capi.Context(W, H, 8, max_frames=NF, lib_path=args.lib)
    n = (NF - 1) * ctx.num_ctus
    d_nodes = {r: torch.zeros(n * 85 * 16, dtype=torch.uint8, device="cuda") for r in (4, 8, 64)}
    d_out = torch.zeros(n * 85 * 16, dtype=torch.uint8, device="cuda")
    for r in (4, 8):   # the nodes the refinement alone starts from
        ctx.motion_search_device(*layout, d_nodes[r].data_ptr(), stream=st, qp=qp, search_range=r)
    ctx.motion_search_pu_wide_device(*layout, d_nodes[64].data_ptr(), None, None, stream=st, qp=qp, search_range=64)
    torch.cuda.synchronize()

    def search(r):
        ctx.motion_search_device(*layout, d_nodes[r].data_ptr(), stream=st, qp=qp, search_range=r)

    def refine(r):
        ctx.motion_refine_device(*layout, d_nodes[r].data_ptr(), d_out.data_ptr(), stream=st, qp=qp, max_range=r)

    out = {"tool": "tools/motion_refine_bench.py", "commit": _commit(args.commit), "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "library": capi.load_library(args.lib).fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "picture_pairs": NF - 1, "ctus_per_launch": n, "qp": qp, "planes": "int16", "clip": "frames.pan_clip"},
           "timing": "per launch; HIP events on the caller's stream around a window of launches ending in a synchronise; ms = median of the windows, "
                     "warmed by two launches; all figures from one process",
           "expectation": "the refinement takes less time than the +-8 SATD search (4 608 tile Hadamards per CTU against 18 496, plus ~1 500 filter "
                          "multiply-adds per tile candidate)"}
    runs = {   # what is launched, and the buffers it writes
        "refine_after_range8": (lambda: refine(8), [d_out]),
        "refine_after_range4": (lambda: refine(4), [d_out]),
        "search_range4_satd": (lambda: search(4), [d_nodes[4]]),
        "search_range8_satd": (lambda: search(8), [d_nodes[8]]),
        "search_range4_plus_refine": (lambda: (search(4), refine(4)), [d_nodes[4], d_out]),
        "search_range8_plus_refine": (lambda: (search(8), refine(8)), [d_nodes[8], d_out]),
        "refine_after_range64": (lambda: refine(64), [d_out]),
    }
    for name, (fn, written) in runs.items():
        out[name] = measure(fn, written)
        r = out[name]
        print(f"{name:28s}: {r['ms']:.3f} ms per launch ({r['ms_min']:.3f} .. {r['ms_max']:.3f})  sha256 {r['sha256'][:16]}", flush=True)
    refine(8)   # the content figures are those of the +-8 nodes
    torch.cuda.synchronize()
    q = np.frombuffer(d_out.cpu().numpy().tobytes(), capi.MOTION_QPEL_DTYPE)
    live = q["cost_best"] != 0xFFFFFFFF
    out["content"] = {"nodes": int(live.sum()), "off_the_integer_grid": float((((q["mvx"] | q["mvy"]) & 3) != 0)[live].mean())}
    below = out["refine_after_range8"]["ms"] < out["search_range8_satd"]["ms"]
    out["checks"] = {"refine_below_search_range8": bool(below),
                     "refine_over_search_range8": out["refine_after_range8"]["ms"] / out["search_range8_satd"]["ms"],
                     "refine_over_search_range4": out["refine_after_range4"]["ms"] / out["search_range4_satd"]["ms"]}
    print("checks:", json.dumps(out["checks"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
