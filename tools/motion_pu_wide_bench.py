#!/usr/bin/env python3
"""Measurement: the PU motion search at HM's SearchRange 64 beside the square wide search on the bench GOP's geometry (64 pictures of 1920 x 1080,
int16 planes at 8 bit resident in HBM: 63 picture pairs = 32 130 CTUs per launch).

Per launch, SAD, search range 64, HIP events on the caller's stream around:
  (a) fhevc_motion_search_device            the 85 square nodes (k_motion_wide.hip: the baseline)
  (b) fhevc_motion_search_pu_wide_device    all three outputs: nodes, 124 PUs, 384 small PUs
  (c) fhevc_motion_search_pu_wide_device    the 124 PUs only
  (d) fhevc_motion_search_pu_wide_device    the 384 small PUs only
  (g) the same call as (b) from a context created under FHEVC_PU_WIDE=generic (the MR = 64 layouts of k_motion_pu.hip and k_motion_pu_small.hip on
      the same 8-bit planes), on --generic-frames pictures only; compared per CTU
All run in ONE process on one device, INTERLEAVED: a round times a, b, c, d, g one after the other, --repeats rounds; every figure is the median over
the rounds with the smallest and largest next to it, and the spread is (largest - smallest) / median.
Two readings, no number fixed in advance: g / b per CTU (the byte path stays only if it is faster than the generic path on the same input), and
b / a with b against c + d (what the 508 PUs cost beside the squares, and whether one launch is worth it).

Needs an MI355X; without one it fails.  Writes profiles/motion_pu_wide.json (--out)."""
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
    ap.add_argument("--generic-frames", type=int, default=3, help="pictures of the generic leg (it is many times slower: compared per CTU)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--range", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7, help="interleaved rounds (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=1, help="launches per timed window")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_pu_wide.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_pu_wide_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, NG, qp, R = args.width, args.height, args.frames, args.generic_frames, args.qp, args.range
    assert 2 <= NG <= NF
    ys = [y.astype(np.int16) for y in frames.pan_clip(W, H, NF)]
    flat, org, stride, fs = frames.guarded_plane(ys, 8, np.int16, margin=80, poison=None)
    planes = torch.from_numpy(flat).cuda()
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (planes.data_ptr() + 2 * org, 2, stride, fs, NF)
    layout_g = (planes.data_ptr() + 2 * org, 2, stride, fs, NG)

    ctx = capi.Context(W, H, 8, max_frames=NF)
    ctx.set_motion_distortion("sad")
    os.environ["FHEVC_PU_WIDE"] = "generic"   # read once, when a context is created
    ctx_g = capi.Context(W, H, 8, max_frames=NF)
    del os.environ["FHEVC_PU_WIDE"]
    n, n_g = (NF - 1) * ctx.num_ctus, (NG - 1) * ctx.num_ctus
    per = {"nodes": 85, "pus": capi.PUS_PER_CTU, "small": capi.PUS_SMALL_PER_CTU}
    buf = lambda count, k: torch.zeros(count * per[k] * 16, dtype=torch.uint8, device="cuda")
    a_nodes = buf(n, "nodes")
    b = {k: buf(n, k) for k in per}
    c_pus, d_small = buf(n, "pus"), buf(n, "small")
    g = {k: buf(n_g, k) for k in per}

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.launches

    def figure(ev, ctus):
        med = statistics.median(ev)
        return {"ms": med, "ms_min": min(ev), "ms_max": max(ev), "spread": (max(ev) - min(ev)) / med, "us_per_ctu": 1000.0 * med / ctus, "ctus_per_launch": ctus,
                "windows": len(ev), "launches_per_window": args.launches}

    kw = dict(stream=st, qp=qp, search_range=R)
    runs = {
        "a_square_nodes": (n, lambda: ctx.motion_search_device(*layout, a_nodes.data_ptr(), **kw)),
        "b_all_three": (n, lambda: ctx.motion_search_pu_wide_device(*layout, b["nodes"].data_ptr(), b["pus"].data_ptr(), b["small"].data_ptr(), **kw)),
        "c_pus_only": (n, lambda: ctx.motion_search_pu_wide_device(*layout, None, c_pus.data_ptr(), None, **kw)),
        "d_small_only": (n, lambda: ctx.motion_search_pu_wide_device(*layout, None, None, d_small.data_ptr(), **kw)),
        "g_generic_all_three": (n_g, lambda: ctx_g.motion_search_pu_wide_device(*layout_g, g["nodes"].data_ptr(), g["pus"].data_ptr(), g["small"].data_ptr(), **kw)),
    }
    for _, fn in runs.values():
        fn()
    torch.cuda.synchronize()
    assert torch.equal(a_nodes, b["nodes"]), "the nodes of the wide PU search differ from the square search's"
    assert torch.equal(c_pus, b["pus"]) and torch.equal(d_small, b["small"]), "a family alone differs from the same family among all three"
    for k in per:
        assert torch.equal(g[k], b[k][:g[k].numel()]), f"the generic path's {k} differ from the byte path's"
    ev = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, (_, fn) in runs.items():
            ev[k].append(window(fn))
    res = {k: figure(v, runs[k][0]) for k, v in ev.items()}
    a, bb, c, d = (res[k]["ms"] for k in ("a_square_nodes", "b_all_three", "c_pus_only", "d_small_only"))
    g_over_b = res["g_generic_all_three"]["us_per_ctu"] / res["b_all_three"]["us_per_ctu"]
    out = {"tool": "tools/motion_pu_wide_bench.py", "commit": _commit(args.commit), "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "picture_pairs": NF - 1, "ctus_per_launch": n, "generic_frames": NG, "qp": qp, "search_range": R,
                        "planes": "int16", "bit_depth": 8, "clip": "frames.pan_clip"},
           "timing": "per launch; HIP events on the caller's stream around a window of launches ending in a synchronise; the legs interleaved round by "
                     "round in one process, each warmed by one launch; ms = median over the rounds; spread = (max - min) / median",
           "runs": res,
           "readings": {"g_over_b_per_ctu": g_over_b, "byte_path_faster_than_generic": bool(g_over_b > 1.0), "b_over_a": bb / a, "c_over_a": c / a, "d_over_a": d / a,
                        "b_over_c_plus_d": bb / (c + d), "largest_spread": max(r["spread"] for r in res.values())}}
    for k, r in res.items():
        print(f"{k:22s}: {r['ms']:9.3f} ms  [{r['ms_min']:.3f} .. {r['ms_max']:.3f}]  {r['us_per_ctu']:8.3f} us/CTU  spread {r['spread']:.3f}", flush=True)
    print(f"g/b per CTU {g_over_b:.2f}  b/a {bb / a:.2f}  c/a {c / a:.2f}  d/a {d / a:.2f}  b/(c+d) {bb / (c + d):.2f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()
    ctx_g.close()


if __name__ == "__main__":
    main()
