#!/usr/bin/env python3
"""TEST/QUALITY INFRASTRUCTURE (uses oracle/_ref/libhmref_p.so).  What the tree decision (fhevc_p_tree_select*) costs in rate and saves in time when its
depth ranges are forced on the reference's own P-picture encode -- reported, never asserted.

The two 832 x 480 clips of eval_p.py (one global pan; two transparent motions), its QPs and its protocol: I P P P, the P pictures at QP + 6, POC >= 2
restricted, BD-rate of the restricted pictures and the time in compressSlice against the unrestricted search.  Variants, all in the same run:
  full_rdo              the anchor
  p_depth_range         fhevc_p_depth_range's maps (the shipped rule, as eval_p.py's motion_rule)
  tree_default          the tree at the default rule: the unfitted hard decision, depth_min == depth_max
  tree_<name>           the tree at a small grid of margins (GRID below)
The tree's maps come from the numpy / Python restatements of the chain (zero-centred SAD search at range 8, quarter-sample refinement, partition-size
selection, tree): tests/test_gpu_p_tree.py holds the library on the GPU to the same bits, so no GPU is needed here.

usage: python tests/quality/eval_p_tree.py [--size 832x480] [--frames 4] [--workers 8] [--json profiles/p_tree_quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))       # tests/: the restatements
import eval_p  # noqa: E402
from eval_rd import bd_rate  # noqa: E402
from fasthevc_amd import capi, frames  # noqa: E402

RANGE = 8
QPS = (22, 27, 32, 37)
# margins per level (64, 32, 16): q8 in 1/256 of the cost they scale
GRID = {
    "tree_soft_1_16": dict(split_q8=16, stop_q8=16),                  # a sixteenth either way
    "tree_soft_1_8": dict(split_q8=32, stop_q8=32),
    "tree_soft_1_4": dict(split_q8=64, stop_q8=64),
    "tree_never_force": dict(split_q8=65535, split_abs=0x7FFFFFFF),   # depth_min = 0 (but for the picture edge): splits are only ever forbidden
    "tree_never_force_stop_1_8": dict(split_q8=65535, split_abs=0x7FFFFFFF, stop_q8=32),
}


def tree_shapes(oracle, cur, ref, qp):
    """the selection's records [numCtus, 85] of one pair through the restatements"""
    import motion_range_sweep as sw
    import motion_refine_pu_ref as rp
    import motion_refine_ref as mr
    import pu_shape_ref as sr
    H, W = cur.shape
    cur, ref = cur.astype(np.int64), ref.astype(np.int64)
    found = sw.PairSweep(oracle, cur, ref, 8, qp, sad=True, rmax=RANGE).records(RANGE)
    cur_flat = np.ascontiguousarray(cur.astype(np.int16)).reshape(-1)
    planes = mr.Planes(ref, 8, RANGE + 8)
    nodes = mr.expected(oracle, cur_flat, 0, W, ref, W, H, 8, qp, found["nodes"], RANGE, planes=planes)
    pu = rp.expected(oracle, cur, ref, 8, qp, found["pu"], RANGE, "pu", planes=planes)
    small = rp.expected(oracle, cur, ref, 8, qp, found["small"], RANGE, "small", planes=planes)
    return sr.select(nodes[None], pu[None], small[None], W, H)[0][0]


def encode_forced(lib, ys, qp, ranges):
    """eval_p.encode_seq's protocol with the ranges of picture f >= 2 given by ranges(f, previous picture's depths) -> (depth_min, depth_max) or None"""
    from oracle import oracle_py as op
    H, W = ys[0].shape
    n = ((W + 63) // 64) * ((H + 63) // 64)
    u = np.full((H // 2, W // 2), 128, np.int16)
    buf, org, stride = frames.to_pel_plane(ys[0], 8)
    d, st = op.rdo_encode(lib, buf, org, stride, W, H, 8, qp, chroma=(u, u))
    out = [(d, {"bits": st["coded_bits"], "psnr_y": st["psnr_y"], "seconds": st["seconds"]})]
    for f in range(1, len(ys)):
        buf, org, stride = frames.to_pel_plane(ys[f], 8)
        forced = ranges(f, out[-1][0]) if ranges is not None and f >= 2 else None
        fmin, fmax = (np.ascontiguousarray(a) for a in forced) if forced is not None else (None, None)
        d1, s1 = np.zeros(n * 256, np.uint8), np.zeros(8)
        rc = lib.href_rdo_encode_next_p(buf.reshape(-1).ctypes.data + 2 * org, u.ctypes.data, u.ctypes.data, stride, W, H, 8, qp + 6, f,
                                        None if fmin is None else fmin.ctypes.data, None if fmax is None else fmax.ctypes.data, d1.ctypes.data, s1.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"href_rdo_encode_next_p failed: {rc}")
        out.append((d1.reshape(n, 256), {"bits": float(s1[6]), "psnr_y": float(10 * np.log10(255.0 * 255.0 / (s1[4] / (W * H)))), "seconds": float(s1[3])}))
    return out


def _run(job):
    """one clip at one slice QP: the anchor and every variant; runs in its own process (HM is single-threaded)"""
    clip, qp, (W, H), nframes, speed = job
    import p_tree_ref as tr
    from oracle import oracle_py as op
    eval_p.CLIP, eval_p.SPEED = clip, speed
    lib, oracle = eval_p.load_p(), op.load_oracle()
    ys = eval_p.pan_clip(W, H, nframes)
    tail = lambda seq: (sum(s["bits"] for _, s in seq[2:]), float(np.mean([s["psnr_y"] for _, s in seq[2:]])), sum(s["seconds"] for _, s in seq[2:]))
    anchor = encode_forced(lib, ys, qp, None)
    out = {"full_rdo": tail(anchor)}
    prule = op.PRule.from_buffer_copy(bytes(capi.p_rule_default()))
    seq = encode_forced(lib, ys, qp, lambda f, prev: eval_p.motion_ranges(oracle, prule, ys[f], ys[f - 1], prev, qp + 6))
    out["p_depth_range"] = tail(seq)
    out["p_depth_range:agreement"] = [float((seq[f][0] == anchor[f][0]).mean()) for f in range(2, nframes)]
    shapes = {f: tree_shapes(oracle, ys[f], ys[f - 1], qp + 6) for f in range(2, nframes)}
    rules = dict({"tree_default": None}, **{name: capi.p_tree_rule(**kw) for name, kw in GRID.items()})
    # the 4x4 units inside the picture: the reference reports depths for the others as well, the maps hold 0 there
    n = ((W + 63) // 64) * ((H + 63) // 64)
    live = np.zeros((n, 16, 16), bool)
    for c in range(n):
        vw, vh = tr.valid_size(c, W, H)
        live[c, :(vh + 3) // 4, :(vw + 3) // 4] = True
    live = live.reshape(n, 256)
    for name, rule in rules.items():
        maps = {f: tr.select(shapes[f][None], W, H, rule=rule) for f in shapes}
        seq = encode_forced(lib, ys, qp, lambda f, prev: (maps[f][1][0], maps[f][2][0]))
        out[name] = tail(seq)
        out[name + ":agreement"] = [float((seq[f][0] == anchor[f][0]).mean()) for f in range(2, nframes)]
        out[name + ":inside"] = [float(((maps[f][1][0] <= anchor[f][0]) & (anchor[f][0] <= maps[f][2][0]))[live].mean()) for f in range(2, nframes)]
    return (clip, qp), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="832x480")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--speed", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "p_tree_quality.json"))
    args = ap.parse_args()
    from multiprocessing import Pool
    W, H = (int(v) for v in args.size.split("x"))
    clips = ("global", "overlaid")
    with Pool(args.workers) as pool:
        res = dict(pool.map(_run, [(clip, qp, (W, H), args.frames, args.speed) for clip in clips for qp in QPS], chunksize=1))
    names = ["p_depth_range", "tree_default"] + list(GRID)
    report = {"tool": "tests/quality/eval_p_tree.py", "protocol": f"{W}x{H}, {args.frames} frames I P P ..., P pictures at QP + 6, POC >= 2 restricted; BD-rate of the restricted "
              "pictures and time in compressSlice against the unrestricted search (eval_p.py's protocol, clips and BD-rate code); tree maps from the "
              f"restatements of the zero-centred chain at range {RANGE}", "qp": list(QPS), "grid": GRID, "clips": {}}
    for clip in clips:
        ra, pa = [res[(clip, q)]["full_rdo"][0] for q in QPS], [res[(clip, q)]["full_rdo"][1] for q in QPS]
        ta = sum(res[(clip, q)]["full_rdo"][2] for q in QPS)
        entry = {"what": "one global pan of a hetero picture" if clip == "global" else "two transparent motions in opposite directions",
                 "full_rdo": [res[(clip, q)]["full_rdo"] for q in QPS], "variants": {}}
        for name in names:
            pts = [res[(clip, q)][name] for q in QPS]
            v = {"points": pts, "bd_rate_percent": bd_rate(ra, pa, [p[0] for p in pts], [p[1] for p in pts]), "compress_slice_time_ratio": ta / sum(p[2] for p in pts),
                 "depth_agreement_with_full_rdo": [float(np.mean(res[(clip, q)][name + ":agreement"])) for q in QPS]}
            if name.startswith("tree"):
                v["full_rdo_depth_inside_the_range"] = [float(np.mean(res[(clip, q)][name + ":inside"])) for q in QPS]
            entry["variants"][name] = v
            print(f"{clip:9s} {name:28s} BD-rate {v['bd_rate_percent']:+7.2f} %   compressSlice {v['compress_slice_time_ratio']:5.2f}x faster", flush=True)
        report["clips"][clip] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.json)


if __name__ == "__main__":
    main()
