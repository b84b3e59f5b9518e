"""Host overhead of the config-4 host forms, one build of the library against another in ONE process (tools/build_variant.sh builds both):

    tools/build_variant.sh HEAD~1 parent && tools/build_variant.sh WORK this
    python tools/host_forms_ab.py build/ab/parent.so build/ab/this.so profiles/host_forms_ab.json

Wall clock per call of fhevc_motion_refine_pu_wide (all three families, max_range 8) and fhevc_p_tree_merge_frame (search_range 8, coarse_range 0) on one
1920 x 1080 8-bit pair; three rounds of parent, this, parent again, ten calls each after two warm-up calls.  The second parent run of a round gives the
band the box has that day: this build passes a round when it lies inside the band or within the band's width beyond it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fasthevc_amd import capi, frames  # noqa: E402

W, H, QP, CALLS, WARMUP, ROUNDS = 1920, 1080, 30, 10, 2, 3


def main(parent_path, this_path, out_path):
    ys = frames.pan_clip(W, H, 2, seed=7, v_structure=3, v_noise=-2)
    (ref, org, stride), (cur, _, _) = frames.to_pel_plane(ys[0], 8), frames.to_pel_plane(ys[1], 8)
    ctxs = {"parent": capi.Context(W, H, 8, lib_path=parent_path), "this": capi.Context(W, H, 8, lib_path=this_path)}
    found = ctxs["parent"].motion_search_pu_wide(cur, ref, org, stride, qp=QP, search_range=8)
    calls = {
        "refine_pu_wide_ms": lambda c: c.motion_refine_pu_wide(cur, ref, org, stride, qp=QP, max_range=8, nodes=found[0], pus=found[1], pus_small=found[2]),
        "p_tree_merge_frame_ms": lambda c: c.p_tree_merge_frame(cur, ref, org, stride, qp=QP, search_range=8, coarse_range=0),
    }
    # the two builds give the same bytes
    for call in calls.values():
        a, b = call(ctxs["parent"]), call(ctxs["this"])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))

    def timed(c):
        res = {}
        for name, call in calls.items():
            for _ in range(WARMUP):
                call(c)
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call(c)
            res[name] = round((time.perf_counter() - t0) * 1e3 / CALLS, 4)
        return res

    rounds, ok = [], True
    for _ in range(ROUNDS):
        r = {"parent": timed(ctxs["parent"]), "this": timed(ctxs["this"]), "parent_again": timed(ctxs["parent"])}
        r["ratio_to_parent_mean"], r["inside"] = {}, {}
        for name in calls:
            lo, hi = sorted((r["parent"][name], r["parent_again"][name]))
            r["ratio_to_parent_mean"][name] = round(2 * r["this"][name] / (lo + hi), 4)
            r["inside"][name] = bool(lo - (hi - lo) <= r["this"][name] <= hi + (hi - lo))
            ok &= r["inside"][name]
        rounds.append(r)
    doc = {"what": __doc__.split("\n\n")[2].replace("\n", " "), "unit": "ms of wall clock per call", "rounds": rounds,
           "reading": "every round of this build lies inside the band of the two parent runs or within its width beyond it" if ok else
                      "a round of this build lies further outside the band of the two parent runs than the band is wide"}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
