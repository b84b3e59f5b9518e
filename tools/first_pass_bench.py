#!/usr/bin/env python3
"""Measurement: the two first-pass kernels on the bench geometry (1920 x 1080, int16 planes resident in HBM, 16 pictures = 8 160 CTUs per launch).

Per launch, two ways: fhevc_kernel_timing (the library's own HIP events around each launch, averaged over the launches of a window) and HIP events on
the caller's stream around a window of warmed launches that ends in a synchronise.  Every figure is the median of --repeats windows with the smallest
and largest next to it.  Measured:
  * the existing 85-node kernel (fhevc_intra_first_pass_device), and the same with the lists selected in it (fhevc_intra_first_pass_candidates_device);
  * the 4x4 kernel (fhevc_intra_first_pass_4x4_device): best only, lists only, both;
  * with --parent-lib: the 85-node kernel of another build of the library (the parent commit's), in the same process on the same device, so that
    "the 85-node kernel's own time did not move" is a statement about one box.
Two statements are recorded (they do not make the tool fail): the 4x4 kernel (both outputs) takes less time than the 85-node kernel, and the 85-node
kernel's time lies within the parent build's run-to-run spread of the parent build's time.

Needs an MI355X; without one it fails.  Writes profiles/first_pass_4x4.json (--out)."""
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


class _ParentContext:
    """The few entry points this tool times, bound by hand on another build of the library: a build older than this one lacks the newest
    symbols, which capi.load_library binds all at once."""

    def __init__(self, path, width, height, max_frames):
        import ctypes as C
        self.C, vp = C, C.c_void_p
        self.lib = C.CDLL(os.path.abspath(path))
        self.lib.fhevc_create.argtypes = [C.POINTER(vp), C.POINTER(capi.Cfg)]
        self.lib.fhevc_destroy.argtypes = [vp]
        self.lib.fhevc_destroy.restype = None
        self.lib.fhevc_enable_kernel_timing.argtypes = [vp, C.c_int]
        self.lib.fhevc_kernel_timing.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        self.lib.fhevc_intra_first_pass_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
        dev = (C.c_int * 1)(0)
        cfg = capi.Cfg(width, height, 8, 64, 3, 1, dev, None, capi.BACKEND_HIP, max_frames)
        self.h, self.rows = vp(), (height + 63) // 64
        assert self.lib.fhevc_create(C.byref(self.h), C.byref(cfg)) == capi.OK
        assert self.lib.fhevc_enable_kernel_timing(self.h, 1) == capi.OK

    def kernel_timing(self, which, reset=False):
        ms, n = self.C.c_double(), self.C.c_uint64()
        assert self.lib.fhevc_kernel_timing(self.h, which, 1 if reset else 0, self.C.byref(ms), self.C.byref(n)) == capi.OK
        return ms.value, n.value

    def intra_first_pass_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_out, stream=None, qp=32):
        assert self.lib.fhevc_intra_first_pass_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, 0, self.rows, qp, d_out, stream) == capi.OK

    def close(self):
        self.lib.fhevc_destroy(self.h)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per figure (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=10, help="launches per window")
    ap.add_argument("--parent-lib", default=None, help="the library built from the parent commit: its 85-node kernel is timed beside this build's")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_pass_4x4.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("first_pass_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp, k = args.width, args.height, args.frames, args.qp, args.candidates
    ys = [frames.texture16_luma(W, H, seed=7, frame=f).astype(np.int16) for f in range(NF)]
    flat, org, stride, fs = frames.guarded_plane(ys, 8, np.int16, margin=80, poison=None)
    planes = torch.from_numpy(flat).cuda()
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (planes.data_ptr() + 2 * org, 2, stride, fs, NF)

    def measure(ctx, fn, slot):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev, lib = [], []
        for _ in range(args.repeats):
            ctx.kernel_timing(slot, reset=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1) / args.launches)
            ms, n = ctx.kernel_timing(slot, reset=True)
            assert n == args.launches, (slot, n)
            lib.append(ms)

        def summary(v):
            return {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "spread_ms": max(v) - min(v)}
        return {"kernel_timing": summary(lib), "events_around_the_call": summary(ev), "windows": args.repeats, "launches_per_window": args.launches}

    ctx = capi.Context(W, H, 8, max_frames=NF)
    ctx.enable_kernel_timing(True)
    n = NF * ctx.num_ctus
    d_nodes = torch.zeros(n * 85 * 16, dtype=torch.uint8, device="cuda")
    d_m85 = torch.zeros(n * 85 * k, dtype=torch.uint8, device="cuda")
    d_best = torch.zeros(n * 256 * 16, dtype=torch.uint8, device="cuda")
    d_modes = torch.zeros(n * 256 * k, dtype=torch.uint8, device="cuda")
    out = {"tool": "tools/first_pass_bench.py", "commit": _commit(args.commit), "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "ctus_per_launch": n, "pus_per_launch": n * 256, "qp": qp, "num_candidates": k, "planes": "int16"},
           "timing": "per launch; kernel_timing = the library's HIP events around each launch, events_around_the_call = HIP events on the caller's stream "
                     "around a window of launches ending in a synchronise; ms = median of the windows, warmed by three launches",
           "expectation": "the 4x4 kernel takes less time than the 85-node kernel (a quarter of the samples per mode, a cheaper Hadamard, no smoothing pass)"}
    runs = {
        "nodes85_best": (lambda: ctx.intra_first_pass_device(*layout, d_nodes.data_ptr(), stream=st, qp=qp), 2),
        "nodes85_lists": (lambda: ctx.intra_first_pass_candidates_device(*layout, d_m85.data_ptr(), stream=st, qp=qp, num_candidates=k), 2),
        "pus4_best": (lambda: ctx.intra_first_pass_4x4_device(*layout, d_best.data_ptr(), None, stream=st, qp=qp, num_candidates=k), 6),
        "pus4_lists": (lambda: ctx.intra_first_pass_4x4_device(*layout, None, d_modes.data_ptr(), stream=st, qp=qp, num_candidates=k), 6),
        "pus4_both": (lambda: ctx.intra_first_pass_4x4_device(*layout, d_best.data_ptr(), d_modes.data_ptr(), stream=st, qp=qp, num_candidates=k), 6),
    }
    for name, (fn, slot) in runs.items():
        out[name] = measure(ctx, fn, slot)
        r = out[name]["kernel_timing"]
        print(f"{name:14s}: {r['ms']:.4f} ms per launch ({r['ms_min']:.4f} .. {r['ms_max']:.4f}); events around the call {out[name]['events_around_the_call']['ms']:.4f} ms", flush=True)
    out["checks"] = {"pus4_both_below_nodes85": out["pus4_both"]["kernel_timing"]["ms"] < out["nodes85_best"]["kernel_timing"]["ms"]}
    if args.parent_lib:
        pctx = _ParentContext(args.parent_lib, W, H, NF)
        out["parent_nodes85_best"] = measure(pctx, lambda: pctx.intra_first_pass_device(*layout, d_nodes.data_ptr(), stream=st, qp=qp), 2)
        out["parent_nodes85_best"]["commit"] = args.parent_commit or "parent"
        # once more in the other order, so that drift between the first and the last measurement of the run shows
        out["nodes85_best_again"] = measure(ctx, runs["nodes85_best"][0], 2)
        p, a, b = (out[x]["kernel_timing"] for x in ("parent_nodes85_best", "nodes85_best", "nodes85_best_again"))
        spread = max(p["spread_ms"], a["spread_ms"], b["spread_ms"])
        out["checks"]["nodes85_did_not_move"] = {"parent_ms": p["ms"], "this_ms": [a["ms"], b["ms"]], "run_to_run_spread_ms": spread,
                                                 "within_spread": min(abs(a["ms"] - p["ms"]), abs(b["ms"] - p["ms"])) <= spread}
        print(f"parent 85-node: {p['ms']:.4f} ms ({p['ms_min']:.4f} .. {p['ms_max']:.4f}); this build {a['ms']:.4f} and {b['ms']:.4f} ms", flush=True)
        pctx.close()
    print("checks:", json.dumps(out["checks"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
