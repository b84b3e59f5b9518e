"""The existing RD entry points, one build of the library against another in ONE process (tools/build_variant.sh builds both):

    tools/build_variant.sh HEAD~1 parent && tools/build_variant.sh WORK this
    python tools/motion_rd_ab.py build/ab/parent.so build/ab/this.so profiles/intra_rd_qt_ab.json

fhevc_motion_rd_device (re-priced nodes with their predictor records) and fhevc_motion_rd_pu_device (part_mode 8) at max_range 8 and 64 on 16 pairs of
1920 x 1080 uint8 planes (8 160 CTUs per call), and fhevc_intra_rd_device (plain, on the first pass's records of the 16 current pictures: the same CTUs;
where both builds have it, fhevc_intra_rd_qt_device at tu_depths 3 on the same records, slot 37, and fhevc_intra_rd_nxn_device on them and the 4x4
first pass's records, slot 39);
the average of ten calls through the library's timing slots 29, 31, 33, 37 and 39, after two warm-up calls; three
interleaved rounds of parent, this, parent again.  The second parent run of a round gives the band the box has that day: this build passes a round when
it lies inside the band or within the band's width beyond it.  Both builds give the same bytes, or nothing is timed."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fasthevc_amd import capi, frames  # noqa: E402

W, H, NF, QP, CALLS, WARMUP, ROUNDS = 1920, 1080, 17, 32, 10, 2, 3
FAM = (85, 124, 384)


def main(parent_path, this_path, out_path):
    import torch
    if not torch.cuda.is_available():
        sys.exit("motion_rd_ab.py needs an MI355X: no GPU is visible")
    P = NF - 1
    ctxs = {"parent": capi.Context(W, H, 8, max_frames=NF, lib_path=parent_path), "this": capi.Context(W, H, 8, max_frames=NF, lib_path=this_path)}
    c0 = ctxs["parent"]
    total = P * c0.num_ctus
    d8 = torch.from_numpy(np.stack(frames.pan_clip(W, H, NF))).cuda()
    buf = lambda per=85, nbytes=16: torch.zeros((total * per * nbytes,), dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    layout = (d8.data_ptr(), 1, W, W * H, NF)
    chain = {}
    for R in (8, 64):      # real records, made once by the parent build
        found, fine, priced, mvp = [buf(f) for f in FAM], [buf(f) for f in FAM], [buf(f) for f in FAM], [buf(f, 8) for f in FAM]
        merge_pu, merge_s, shapes = buf(124), buf(384), buf()
        c0.motion_search_pu_wide_device(*layout, *[p(t) for t in found], qp=QP, search_range=R)
        c0.motion_refine_pu_wide_device(*layout, p(found[0]), p(fine[0]), p(found[1]), p(fine[1]), p(found[2]), p(fine[2]), qp=QP, max_range=R)
        c0.motion_amvp_device(NF, *[p(t) for t in fine], *[p(t) for t in priced], *[p(t) for t in mvp], qp=QP)
        c0.motion_merge_pu_device(*layout, p(priced[0]), p(merge_pu), p(merge_s), qp=QP, max_range=R)
        c0.pu_shape_select_merge_device(*[p(t) for t in priced], p(merge_pu), p(merge_s), P, p(shapes))
        torch.cuda.synchronize()
        del found, fine
        chain[R] = (priced, mvp, c0.rd_pu_inputs(p(priced[0]), p(priced[1]), p(priced[2]), p(merge_pu), p(merge_s), p(mvp[0]), p(mvp[1]), p(mvp[2]), p(shapes)),
                    (merge_pu, merge_s, shapes))
    out = buf()
    first = buf()
    current = (d8.data_ptr() + W * H, 1, W, W * H, P)   # the current picture of every pair
    c0.intra_first_pass_device(*current, p(first), qp=QP)
    torch.cuda.synchronize()
    calls = {"intra_rd_ms": (33, lambda c: c.intra_rd_device(*current, p(first), p(out), qp=QP))}
    if all(hasattr(c.lib, "fhevc_intra_rd_qt_device") for c in ctxs.values()):   # both builds have the intra instances of three TU depths: slot 37
        calls["intra_rd_qt_3_ms"] = (37, lambda c: c.intra_rd_qt_device(*current, p(first), 3, p(out), qp=QP))
    if all(hasattr(c.lib, "fhevc_intra_rd_nxn_device") for c in ctxs.values()):  # both builds have the instances with the NxN candidate: slot 39
        first4 = buf(256)
        c0.intra_first_pass_4x4_device(*current, p(first4), None, qp=QP, num_candidates=0)
        torch.cuda.synchronize()
        calls["intra_rd_nxn_ms"] = (39, lambda c: c.intra_rd_nxn_device(*current, p(first), p(first4), p(out), qp=QP))
    for R in (8, 64):
        priced, mvp, inputs, _ = chain[R]
        calls[f"rd_{R}_ms"] = (29, lambda c, R=R, q=priced, v=mvp: c.motion_rd_device(*layout, capi.RD_SOURCE_EXPLICIT, p(q[0]), p(out), d_mvp=p(v[0]), qp=QP, max_range=R))
        calls[f"rd_pu_{R}_ms"] = (31, lambda c, R=R, i=inputs: c.motion_rd_pu_device(*layout, 8, i, p(out), qp=QP, max_range=R))
    # the two builds give the same bytes
    for name, (_, call) in calls.items():
        got = []
        for c in ctxs.values():
            out.zero_()
            call(c)
            torch.cuda.synchronize()
            got.append(out.cpu().numpy().tobytes())
        assert got[0] == got[1], name

    def timed(c):
        res = {}
        c.enable_kernel_timing(True)
        for name, (slot, call) in calls.items():
            for _ in range(WARMUP):
                call(c)
            torch.cuda.synchronize()
            c.kernel_timing(slot, reset=True)
            for _ in range(CALLS):
                call(c)
            torch.cuda.synchronize()
            ms, count = c.kernel_timing(slot, reset=True)
            assert count == CALLS
            res[name] = round(ms, 4)
        c.enable_kernel_timing(False)
        return res

    rounds = []
    for _ in range(ROUNDS):
        rounds.append({"parent": timed(ctxs["parent"]), "this": timed(ctxs["this"]), "parent_again": timed(ctxs["parent"])})
        print(json.dumps(rounds[-1]), flush=True)
    verdict = {}
    for name in calls:
        inside = []
        for r in rounds:
            a, b, t = r["parent"][name], r["parent_again"][name], r["this"][name]
            lo, hi, width = min(a, b), max(a, b), abs(a - b)
            inside.append(lo - width <= t <= hi + width)
        mean = lambda k: sum(r[k][name] for r in rounds) / len(rounds)
        verdict[name] = {"this_to_parent": round(mean("this") / mean("parent"), 4), "parent_again_to_parent": round(mean("parent_again") / mean("parent"), 4),
                         "rounds_inside_the_band_or_within_its_width_beyond": int(sum(inside)), "rounds": len(rounds)}
    res = {"what": "existing RD entry points, parent commit against this one: fhevc_motion_rd_device (re-priced nodes with predictor records) and fhevc_motion_rd_pu_device "
                   "(part_mode 8) at max_range 8 and 64, fhevc_intra_rd_device (plain) and, where both builds have it, fhevc_intra_rd_qt_device at tu_depths 3 (plain, slot 37), uint8 planes, 16 pairs of 1920x1080 (8 160 CTUs) per call; average of 10 calls "
                   "per run through the library's timing slots 29, 31, 33 and -- fhevc_intra_rd_qt_device at tu_depths 3 and fhevc_intra_rd_nxn_device with the 4x4 first pass's records, where both builds have them -- 37 and 39; three interleaved rounds of parent, this commit, parent again (the second parent run gives the noise band) in one process on one MI355X",
           "unit": "ms per call", "same_bytes_from_both_builds": True, "rounds": rounds, "verdict": verdict}
    print(json.dumps(verdict), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main(*sys.argv[1:4])
