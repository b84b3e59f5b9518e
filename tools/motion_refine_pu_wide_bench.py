#!/usr/bin/env python3
"""Measurement: the quarter-sample refinement of the PUs laid out for vectors up to +-64 (fhevc_motion_refine_pu_wide, the MR = 64 instances of
k_motion_refine_pu.hip) beside the MR = 8 layout the library had before, on the bench GOP's geometry (64 pictures of 1920 x 1080, int16 planes at
8 bit resident in HBM: 63 picture pairs = 32 130 CTUs per launch) of a pan clip whose two motions exceed 8 samples per picture.

Per launch, HIP events on the caller's stream around:
  (a) fhevc_motion_refine_pu_device at max_range 8 on the +-8 searches' vectors      the existing code: the baseline
  (b) fhevc_motion_refine_pu_wide_device, PUs only, max_range 64, THE SAME vectors   same arithmetic, the 80 016 B window: the window's cost
  (c) the same on the wide search's own vectors (+-64)                               long vectors: windows that reach further into the picture
  (d) the same, all three families                                                   + the launch of the square kernel
  (e) fhevc_motion_refine_device at max_range 64 on the wide search's nodes          the squares alone: existing code
  (f) fhevc_motion_search_pu_wide_device at +-64 and (d) on one stream               what a caller pays for all 593 quarter-sample costs of a CTU
and, for the staging of only the part of the window that max_range reaches, (b) at max_range 9 and 33 from the default context (part) and from a
context created under FHEVC_REFINE_PU_STAGE=full (whole window); at max_range 64 the part is the whole window.
All run in ONE process on one device, INTERLEAVED: a round times every run one after the other, --repeats rounds; every figure is the median over
the rounds with the smallest and largest next to it, and the spread is (largest - smallest) / median.
Also recorded: what hipOccupancyMaxActiveBlocksPerMultiprocessor answers for the MR = 64 instance (two workgroups of 80 016 + 224 B are 160 480 of
the CU's 163 840 B: by arithmetic they fit with nothing to spare) and the cap of the persistent grid that follows from it.
No time is required.  The expectation from a count of the code is b / a a little above 1: the same 26 x 18 tile predictions per CTU, plus 80 KB
instead of 15.5 KB staged per CTU; the measured b / a and c / b are recorded next to it.

Needs an MI355X; without one it fails.  Writes profiles/motion_refine_pu_wide.json (--out)."""
import argparse
import ctypes as C
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
    ap.add_argument("--speeds", type=int, nargs=2, default=(19, -27), help="samples per picture of the clip's two overlaid motions")
    ap.add_argument("--repeats", type=int, default=7, help="interleaved rounds (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=2, help="launches per timed window")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_refine_pu_wide.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_refine_pu_wide_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    ys = [y.astype(np.int16) for y in frames.pan_clip(W, H, NF, v_structure=args.speeds[0], v_noise=args.speeds[1])]
    flat, org, stride, fs = frames.guarded_plane(ys, 8, np.int16, margin=80, poison=None)
    planes = torch.from_numpy(flat).cuda()
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (planes.data_ptr() + 2 * org, 2, stride, fs, NF)

    ctx = capi.Context(W, H, 8, max_frames=NF)
    os.environ["FHEVC_REFINE_PU_STAGE"] = "full"   # read once, when a context is created
    ctx_full = capi.Context(W, H, 8, max_frames=NF)
    del os.environ["FHEVC_REFINE_PU_STAGE"]
    n = (NF - 1) * ctx.num_ctus
    buf = lambda per: torch.zeros(n * per * 16, dtype=torch.uint8, device="cuda")
    PER = (85, capi.PUS_PER_CTU, capi.PUS_SMALL_PER_CTU)
    s8, s64, q = [buf(p) for p in PER], [buf(p) for p in PER], [buf(p) for p in PER]   # the +-8 searches' vectors, the wide search's, the outputs
    ctx.set_motion_distortion("sad")
    ctx.motion_search_pu_device(*layout, s8[1].data_ptr(), s8[0].data_ptr(), stream=st, qp=qp, search_range=8)
    ctx.motion_search_pu_small_device(*layout, s8[2].data_ptr(), stream=st, qp=qp, search_range=8)
    search_wide = lambda: ctx.motion_search_pu_wide_device(*layout, s64[0].data_ptr(), s64[1].data_ptr(), s64[2].data_ptr(), stream=st, qp=qp, search_range=64)
    search_wide()
    torch.cuda.synchronize()
    longest = {}
    for name, t, per in zip(("nodes", "pus", "pus_small"), s64, PER):
        a = t.cpu().numpy().view(capi.MOTION_DTYPE)
        valid = a["cost_best"] != 0xFFFFFFFF
        longest[name] = {"valid": int(valid.sum()), "share_with_a_component_above_8": float((np.maximum(np.abs(a["mvx"].astype(np.int64)), np.abs(a["mvy"].astype(np.int64)))[valid] > 8).mean())}

    lib = capi.load_library()
    lib.fhevc_debug_refine_pu_wide_residency.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    per_cu, cap = C.c_int(0), C.c_int(0)
    assert lib.fhevc_debug_refine_pu_wide_residency(ctx.h, 2, C.byref(per_cu), C.byref(cap)) == capi.OK
    residency = {"instance": "fhevc_motion_refine_pu_kernel<int16_t, packed, MR = 64>", "dynamic_lds_bytes": 80016, "static_lds_bytes": 224, "threads": 256,
                 "hipOccupancyMaxActiveBlocksPerMultiprocessor": per_cu.value, "persistent_grid_cap": cap.value,
                 "arithmetic": "2 * (80 016 + 224) = 160 480 B of the CU's 163 840 B; 218 VGPRs (compiler's report): two waves per SIMD"}

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

    def wide(c, src, max_range, nodes=False):
        c.motion_refine_pu_wide_device(*layout, src[0].data_ptr() if nodes else None, q[0].data_ptr() if nodes else None, src[1].data_ptr(), q[1].data_ptr(),
                                       src[2].data_ptr(), q[2].data_ptr(), stream=st, qp=qp, max_range=max_range)

    def search_then_refine():
        search_wide()
        wide(ctx, s64, 64, nodes=True)

    runs = {
        "a_refine_pu_mr8_on_8": lambda: ctx.motion_refine_pu_device(*layout, s8[1].data_ptr(), q[1].data_ptr(), s8[2].data_ptr(), q[2].data_ptr(), stream=st, qp=qp, max_range=8),
        "b_wide_pus_mr64_on_8": lambda: wide(ctx, s8, 64),
        "c_wide_pus_mr64_on_64": lambda: wide(ctx, s64, 64),
        "d_wide_all_families_mr64_on_64": lambda: wide(ctx, s64, 64, nodes=True),
        "e_refine_square_mr64_on_64": lambda: ctx.motion_refine_device(*layout, s64[0].data_ptr(), q[0].data_ptr(), stream=st, qp=qp, max_range=64),
        "f_search_wide_and_d": search_then_refine,
        "g_wide_pus_mr9_on_8_part": lambda: wide(ctx, s8, 9),
        "g_wide_pus_mr9_on_8_whole": lambda: wide(ctx_full, s8, 9),
        "h_wide_pus_mr33_on_8_part": lambda: wide(ctx, s8, 33),
        "h_wide_pus_mr33_on_8_whole": lambda: wide(ctx_full, s8, 33),
    }
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, fn in runs.items():
            ev[k].append(window(fn))
    res = {k: figure(v) for k, v in ev.items()}
    ms = {k: v["ms"] for k, v in res.items()}
    a, b, c, d, e, f = (ms[k] for k in list(runs)[:6])
    out = {"tool": "tools/motion_refine_pu_wide_bench.py", "commit": _commit(args.commit), "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "library": lib.fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "picture_pairs": NF - 1, "ctus_per_launch": n, "qp": qp, "planes": "int16", "bit_depth": 8,
                        "clip": f"frames.pan_clip(v_structure={args.speeds[0]}, v_noise={args.speeds[1]})",
                        "inputs": "on_8: what the +-8 PU searches wrote (SAD mode); on_64: what fhevc_motion_search_pu_wide wrote at +-64", "wide_search_vectors": longest},
           "timing": "per launch; HIP events on the caller's stream around a window of launches ending in a synchronise; all runs interleaved round by round in "
                     "one process, each warmed by one launch; ms = median over the rounds; spread = (max - min) / median",
           "baseline": "(a) fhevc_motion_refine_pu_device at max_range 8: the MR = 8 instance, the code the parent commit had",
           "expectation": "b / a a little above 1 (the same 26 x 18 tile predictions; 80 KB instead of 15.5 KB staged per CTU); recorded, not required",
           "residency": residency,
           "runs": res,
           "checks": {"b_over_a": b / a, "c_over_b": c / b, "d_minus_c_ms": d - c, "e_ms": e, "f_minus_d_ms": f - d,
                      "part_over_whole_at_9": ms["g_wide_pus_mr9_on_8_part"] / ms["g_wide_pus_mr9_on_8_whole"],
                      "part_over_whole_at_33": ms["h_wide_pus_mr33_on_8_part"] / ms["h_wide_pus_mr33_on_8_whole"],
                      "part_at_9_over_a": ms["g_wide_pus_mr9_on_8_part"] / a,
                      "largest_spread": max(v["spread"] for v in res.values())}}
    for k, v in res.items():
        print(f"{k:34s}: {v['ms']:.3f} ms  (min {v['ms_min']:.3f}, max {v['ms_max']:.3f})", flush=True)
    print(f"b/a {b / a:.2f} (expected a little above 1)  c/b {c / b:.2f}  occupancy answer {per_cu.value}, grid cap {cap.value}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    ctx.close()
    ctx_full.close()


if __name__ == "__main__":
    main()
