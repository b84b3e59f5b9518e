#!/usr/bin/env python3
"""Measurement: the P-picture decision on the device (fhevc_p_depth_range_device, k_p_rule.hip) on the bench GOP's geometry.

64 pictures of frames.pan_clip at 1080p resident in HBM (uint8 planes), reference maps = the classifier's depth maps of the same GOP, so 63 P
pictures = 32 130 CTUs per call.  Everything is timed with HIP events on one explicit stream around warmed, repeated launches that end in a
synchronise; every figure is the median of --repeats such windows, with the smallest and largest next to it.  Reported:
  * the rule kernel alone, per prev_mode: ms, the bytes the pass needs computed from shapes (nodes + reference-map bytes read + maps written)
    over that time, and that rate as a share of the 8 TB/s HBM peak.  A pass this small is partly launch-bound: the share is a record, not a goal;
  * the motion search alone and search + rule queued on one stream, for +-4 SATD (default rule, co-located) and +-64 SAD (wide rule, node mode),
    with the spread (largest - smallest window) of the search-alone runs;
  * INFORMATIVE ONLY: the old route for the same GOP -- download the nodes, the host functions per CTU, upload the two maps.  The host functions
    are called through ctypes, so the figure includes ctypes call overhead (and numpy slicing) per CTU; it is not a measurement of the C code alone.
Two statements are checked and recorded (they do not make the tool fail): the rule kernel takes less time than the +-4 search of the same batch, and
search + rule on one stream take no more than search alone + rule alone + the spread of the search-alone runs.

Needs an MI355X; without one it fails.  Writes profiles/p_rule_device.json (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fasthevc_amd import capi, frames, weights  # noqa: E402

HBM_PEAK = 8.0e12
MAP_BYTES_READ = {"colocated": 256, "unit": 256, "node": 21}   # per CTU: its own map; one byte per 4x4 unit; one byte per node asked (at most 1 + 4 + 16)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per figure (median, smallest, largest)")
    ap.add_argument("--launches", type=int, default=20, help="launches per window of the rule kernel and the +-4 search (the +-64 search: a fifth)")
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p_rule_device.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("p_rule_bench.py needs an MI355X: no GPU is visible")
    W, H, NF, qp = args.width, args.height, args.frames, args.qp
    P = NF - 1
    ctx = capi.Context(W, H, 8, weights.random_weights(0), max_frames=NF)
    n = ctx.num_ctus
    ys = np.stack(frames.pan_clip(W, H, NF))
    d8 = torch.from_numpy(ys).cuda()
    d_maps = torch.zeros((NF, n, 256), dtype=torch.uint8, device="cuda")
    d_nodes = torch.zeros((P, n, 85, 16), dtype=torch.uint8, device="cuda")
    d_min = torch.zeros((P, n, 256), dtype=torch.uint8, device="cuda")
    d_max = torch.zeros((P, n, 256), dtype=torch.uint8, device="cuda")
    ts = torch.cuda.Stream()   # an explicit stream: a NULL handle means the library's own stream, which torch events do not see
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    layout = (d8.data_ptr(), 1, W, W * H, NF)

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    def measure(fn, launches):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = [window(fn, launches) for _ in range(args.repeats)]
        return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "spread_ms": max(ms) - min(ms), "windows": len(ms), "launches_per_window": launches}

    ctx.predict_frames_device(*layout, d_maps.data_ptr(), stream=st, qp=qp)
    torch.cuda.synchronize()
    out = {"tool": "tools/p_rule_bench.py", "device": torch.cuda.get_device_name(0), "library": capi.load_library().fhevc_version().decode(),
           "geometry": {"width": W, "height": H, "frames": NF, "p_pictures": P, "ctus_per_picture": n, "ctus": P * n, "qp": qp, "planes": "uint8"},
           "timing": "HIP events on one stream around warmed, repeated launches ending in a synchronise; ms = median of the windows",
           "rule_alone": {}, "chains": {}}
    settings = {"range4_satd": dict(search_range=4, sad=False, mode="colocated", rule=capi.p_rule_default(), rule_name="default", launches=args.launches),
                "range64_sad": dict(search_range=64, sad=True, mode="node", rule=capi.p_rule_default_wide(), rule_name="wide", launches=max(2, args.launches // 5))}
    for name, s in settings.items():
        ctx.set_motion_distortion("sad" if s["sad"] else "satd")

        def search(s=s):
            ctx.motion_search_device(*layout, d_nodes.data_ptr(), stream=st, qp=qp, search_range=s["search_range"])

        def rule(s=s, mode=None):
            ctx.p_depth_range_device(d_nodes.data_ptr(), d_maps.data_ptr(), P, d_min.data_ptr(), d_max.data_ptr(), stream=st, qp=qp,
                                     prev_mode=mode or s["mode"], rule=s["rule"])

        def both():
            search()
            rule()

        search()
        torch.cuda.synchronize()
        if name == "range4_satd":   # the rule kernel alone, per mode, on the nodes of the +-4 search
            for mode in ("colocated", "unit", "node"):
                r = measure(lambda mode=mode: rule(mode=mode), args.launches)
                nbytes = P * n * (85 * 16 + MAP_BYTES_READ[mode] + 512)
                r.update(bytes_from_shapes=nbytes, bytes_per_ctu=nbytes // (P * n), tb_per_s=nbytes / (r["ms"] * 1e-3) / 1e12,
                         share_of_8_tb_per_s_hbm_peak=nbytes / (r["ms"] * 1e-3) / HBM_PEAK, mctu_per_s=P * n / (r["ms"] * 1e-3) / 1e6,
                         note="a pass this small is partly launch-bound; the share is a record, not a criterion")
                out["rule_alone"][mode] = r
                print(f"rule alone, {mode:9s}: {r['ms'] * 1e3:8.1f} us  ({r['ms_min'] * 1e3:.1f} .. {r['ms_max'] * 1e3:.1f})  {r['tb_per_s']:.2f} TB/s from shapes = "
                      f"{100 * r['share_of_8_tb_per_s_hbm_peak']:.1f} % of the 8 TB/s peak", flush=True)
        a, r, b = measure(search, s["launches"]), measure(rule, args.launches), measure(both, s["launches"])
        bound = a["ms"] + r["ms"] + a["spread_ms"]
        out["chains"][name] = {"search_range": s["search_range"], "distortion": "sad" if s["sad"] else "satd", "prev_mode": s["mode"], "rule": s["rule_name"],
                               "search_alone": a, "rule_alone": r, "search_plus_rule_one_stream": b, "sum_plus_search_spread_ms": bound,
                               "chain_within_sum_plus_spread": b["ms"] <= bound}
        print(f"{name}: search alone {a['ms']:.3f} ms (spread {a['spread_ms']:.3f}), rule alone {r['ms']:.3f} ms, search + rule {b['ms']:.3f} ms "
              f"(bound {bound:.3f} ms: {'within' if b['ms'] <= bound else 'ABOVE'})", flush=True)
    out["checks"] = {"rule_kernel_below_range4_search": max(v["ms"] for v in out["rule_alone"].values()) < out["chains"]["range4_satd"]["search_alone"]["ms"],
                     "search_plus_rule_within_sum_plus_spread": {k: v["chain_within_sum_plus_spread"] for k, v in out["chains"].items()}}
    print("checks:", json.dumps(out["checks"]), flush=True)

    if not args.no_host_route:
        # INFORMATIVE ONLY: what a caller did before -- nodes to the host, the host functions per CTU (through ctypes), the two maps back
        ctx.set_motion_distortion("satd")
        ctx.motion_search_device(*layout, d_nodes.data_ptr(), stream=st, qp=qp, search_range=4)
        torch.cuda.synchronize()
        h_nodes = torch.empty((P, n, 85, 16), dtype=torch.uint8).pin_memory()
        h_maps = d_maps.cpu().numpy()
        t0 = time.perf_counter()
        h_nodes.copy_(d_nodes)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        nodes = h_nodes.numpy().view(capi.MOTION_DTYPE).reshape(P, n, 85)
        rule = capi.p_rule_default()
        hmin, hmax = np.zeros((P, n, 256), np.uint8), np.zeros((P, n, 256), np.uint8)
        for p in range(P):
            hmin[p], hmax[p] = capi.p_depth_range(nodes[p], h_maps[p], W, H, qp, rule)
        t2 = time.perf_counter()
        d_min.copy_(torch.from_numpy(hmin))
        d_max.copy_(torch.from_numpy(hmax))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        ctx.p_depth_range_device(d_nodes.data_ptr(), d_maps.data_ptr(), P, d_max.data_ptr(), None, stream=st, qp=qp, prev_mode="colocated", rule=rule)
        torch.cuda.synchronize()
        out["host_route_informative_only"] = {
            "what": "co-located mode, default rule: download of the nodes, fhevc_p_depth_range per CTU, upload of both maps; host clock, one run",
            "caveat": "the host functions are called per CTU through ctypes from Python: the figure includes that call overhead and numpy slicing, not the C code alone",
            "download_nodes_ms": (t1 - t0) * 1e3, "host_functions_ms": (t2 - t1) * 1e3, "upload_maps_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3,
            "device_depth_min_equals_host": bool(np.array_equal(d_max.cpu().numpy(), hmin))}
        print("host route (informative only, includes ctypes overhead):", json.dumps(out["host_route_informative_only"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ctx.close()


if __name__ == "__main__":
    main()
