#!/usr/bin/env python3
"""Measurement: the chain around a coarse per-CTU centre (fhevc_motion_centres, fhevc_motion_search_pu_centred, fhevc_motion_refine_pu_centred) beside the
chain around the zero vector at HM's SearchRange, on the bench GOP's geometry (64 pictures of 1920 x 1080, int16 planes at 8 bit resident in HBM: 63
picture pairs = 32 130 CTUs per launch) of a pan clip whose two motions exceed 8 samples per picture (tools/motion_refine_pu_wide_bench.py's clip).

Per launch, HIP events on the caller's stream around:
  (a) fhevc_motion_centres_device at coarse_range 14                                          the new kernel
  (b) fhevc_motion_search_pu_centred_device at +-8 around (a)'s centres, all three families   the MR = 8 layouts with a per-CTU origin
  (c) fhevc_motion_refine_pu_centred_device at max_range 8 on (b)'s vectors, all three        the MR = 8 refinements staged around the centre
  (d) a + b + c on one stream                                                                 what a caller pays for the 593 quarter-sample costs of a CTU
  (e) fhevc_motion_search_pu_wide_device at +-64 and fhevc_motion_refine_pu_wide_device at 64 the chain it is meant to replace
  (f) the zero-centred +-8 chain: fhevc_motion_search_pu_wide_device and fhevc_motion_refine_pu_wide_device at 8; f_search and f_refine apart as well
All run in ONE process on one device, INTERLEAVED: a round times every run one after the other, --repeats rounds; every figure is the median over the
rounds with the smallest and largest next to it, and the spread is (largest - smallest) / median.
Ratios: d / e (the speed the centre buys), a / b (whether the coarse kernel costs more than the search it feeds), b / f_search and c / f_refine (what the
per-CTU origin costs).  Reported per family, not asserted: the share of valid entries whose refined vector equals leg (e)'s, and the mean cost_best of both
chains over the entries valid in both.  No time is required.

Needs an MI355X; without one it fails.  Writes profiles/motion_centred.json (--out)."""
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

MARKER = 0xFFFFFFFF


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
    ap.add_argument("--coarse-range", type=int, default=14)
    ap.add_argument("--repeats", type=int, default=7, help="interleaved rounds (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=2, help="launches per timed window")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_centred.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_centred_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, Rc = args.width, args.height, args.frames, args.qp, args.coarse_range
    ys = [y.astype(np.int16) for y in frames.pan_clip(W, H, NF, v_structure=args.speeds[0], v_noise=args.speeds[1])]
    flat, org, stride, fs = frames.guarded_plane(ys, 8, np.int16, margin=80, poison=None)
    planes = torch.from_numpy(flat).cuda()
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (planes.data_ptr() + 2 * org, 2, stride, fs, NF)

    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = (NF - 1) * ctx.num_ctus
    buf = lambda per: torch.zeros(n * per * 16, dtype=torch.uint8, device="cuda")
    PER = (85, capi.PUS_PER_CTU, capi.PUS_SMALL_PER_CTU)
    FAMS = ("nodes", "pus", "pus_small")
    cen = buf(1)
    ic, qc = [buf(p) for p in PER], [buf(p) for p in PER]      # the centred chain: integer vectors, refined entries
    iw, qw = [buf(p) for p in PER], [buf(p) for p in PER]      # the chain around zero at 64
    i8, q8 = [buf(p) for p in PER], [buf(p) for p in PER]      # ... and at 8
    ptrs = lambda a: [t.data_ptr() for t in a]
    pairs = lambda a, b: [p for x, y in zip(a, b) for p in (x.data_ptr(), y.data_ptr())]

    centres = lambda: ctx.motion_centres_device(*layout, cen.data_ptr(), stream=st, qp=qp, coarse_range=Rc)
    search_c = lambda: ctx.motion_search_pu_centred_device(*layout, cen.data_ptr(), *ptrs(ic), stream=st, qp=qp, search_range=8)
    refine_c = lambda: ctx.motion_refine_pu_centred_device(*layout, cen.data_ptr(), *pairs(ic, qc), stream=st, qp=qp, max_range=8)
    search_w = lambda R, dst: ctx.motion_search_pu_wide_device(*layout, *ptrs(dst), stream=st, qp=qp, search_range=R)
    refine_w = lambda R, src, dst: ctx.motion_refine_pu_wide_device(*layout, *pairs(src, dst), stream=st, qp=qp, max_range=R)

    def chain_c():
        centres()
        search_c()
        refine_c()

    def chain_w():
        search_w(64, iw)
        refine_w(64, iw, qw)

    def chain_8():
        search_w(8, i8)
        refine_w(8, i8, q8)

    runs = {"a_centres": centres, "b_search_centred": search_c, "c_refine_centred": refine_c, "d_chain_centred": chain_c, "e_chain_wide_64": chain_w,
            "f_chain_zero_8": chain_8, "f_search_zero_8": lambda: search_w(8, i8), "f_refine_zero_8": lambda: refine_w(8, i8, q8)}
    for fn in (chain_c, chain_w, chain_8):      # every buffer holds its chain's output before anything is timed
        fn()
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

    ev = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, fn in runs.items():
            ev[k].append(window(fn))
    res = {k: figure(v) for k, v in ev.items()}
    ms = {k: v["ms"] for k, v in res.items()}

    # what the two chains found: reported, not asserted
    c_rec = cen.cpu().numpy().view(capi.MOTION_DTYPE)
    agreement = {"centres": {"nonzero_share": float(((c_rec["mvx"] != 0) | (c_rec["mvy"] != 0)).mean()),
                             "largest_component": int(max(np.abs(c_rec["mvx"].astype(np.int64)).max(), np.abs(c_rec["mvy"].astype(np.int64)).max()))}}
    for name, a, b in zip(FAMS, qc, qw):
        x, y = a.cpu().numpy().view(capi.MOTION_QPEL_DTYPE), b.cpu().numpy().view(capi.MOTION_QPEL_DTYPE)
        both = (x["cost_best"] != MARKER) & (y["cost_best"] != MARKER)
        agreement[name] = {"valid_in_both": int(both.sum()), "valid_wide_only": int(((y["cost_best"] != MARKER) & ~both).sum()),
                           "same_refined_vector_share": float(((x["mvx"] == y["mvx"]) & (x["mvy"] == y["mvy"]))[both].mean()) if both.any() else None,
                           "mean_cost_best_centred": float(x["cost_best"][both].astype(np.float64).mean()) if both.any() else None,
                           "mean_cost_best_wide_64": float(y["cost_best"][both].astype(np.float64).mean()) if both.any() else None}

    lib = capi.load_library()
    out = {"tool": "tools/motion_centred_bench.py", "commit": _commit(args.commit), "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "library": lib.fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "picture_pairs": NF - 1, "ctus_per_launch": n, "qp": qp, "planes": "int16", "bit_depth": 8,
                        "coarse_range": Rc, "clip": f"frames.pan_clip(v_structure={args.speeds[0]}, v_noise={args.speeds[1]})"},
           "timing": "per launch (legs d, e, f: per chain); HIP events on the caller's stream around a window of launches ending in a synchronise; all runs "
                     "interleaved round by round in one process, each warmed by one launch; ms = median over the rounds; spread = (max - min) / median",
           "runs": res,
           "ratios": {"d_over_e": ms["d_chain_centred"] / ms["e_chain_wide_64"], "a_over_b": ms["a_centres"] / ms["b_search_centred"],
                      "b_over_f_search": ms["b_search_centred"] / ms["f_search_zero_8"], "c_over_f_refine": ms["c_refine_centred"] / ms["f_refine_zero_8"],
                      "d_over_f": ms["d_chain_centred"] / ms["f_chain_zero_8"], "largest_spread": max(v["spread"] for v in res.values())},
           "agreement_with_the_wide_chain": agreement,
           "asserted": "nothing: the shares and mean costs are reported only"}
    for k, v in res.items():
        print(f"{k:20s}: {v['ms']:.3f} ms  (min {v['ms_min']:.3f}, max {v['ms_max']:.3f})", flush=True)
    print(" ".join(f"{k} {v:.3f}" for k, v in out["ratios"].items()), flush=True)
    for name in FAMS:
        print(name, agreement[name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
