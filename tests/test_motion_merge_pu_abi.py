"""The C-ABI surface of the merge stage per PU and of the partition-size selection that takes its costs (no GPU needed: the library loads without one for
context-free functions): the five entry points in the header, in the Python mirror and among the exports, calls rejected before a device is touched,
timing slots 21 and 20, and fhevc_pu_shape_select_merge against the Python restatement of tests/motion_merge_pu_ref.py on random CTUs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import motion_merge_pu_ref as mpr
import pu_shape_ref as sr
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_motion_merge_pu_device": 14, "fhevc_motion_merge_pu": 9, "fhevc_pu_shape_select_merge": 11, "fhevc_pu_shape_select_merge_device": 14,
       "fhevc_p_tree_merge_pu_frame": 13}
GEOMETRIES = [(64, 64), (64, 64), (64, 64), (40, 64), (64, 12), (36, 40), (8, 8), (12, 36)]
CANARY = 0xA5
MARK = mpr.MARK


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def host_select(nodes, pus, small, mpus, msmall, vw, vh, rule, want_costs=True, want_merged=True):
    """fhevc_pu_shape_select_merge on one CTU -> (rc, records, costs, merged), None for an output not asked for; outputs between canaries"""
    lib = capi.load_library()
    bufs = [np.full(n + 32, CANARY, np.uint8) for n in (85 * 16, 85 * 32, 85 * 2)]
    want = (True, want_costs, want_merged)
    keep = [None if a is None else np.ascontiguousarray(a) for a in (nodes, pus, small, mpus, msmall)]
    rc = lib.fhevc_pu_shape_select_merge(*[None if a is None else a.ctypes.data for a in keep], vw, vh, C.byref(rule) if rule is not None else None,
                                         *[b.ctypes.data + 16 if w else None for b, w in zip(bufs, want)])
    for b, w in zip(bufs, want):
        assert (b[:16] == CANARY).all() and (b[-16:] == CANARY).all(), "a canary around an output was written"
        if not w or rc != capi.OK:
            assert (b == CANARY).all(), "an output that was not asked for, or of a rejected call, was written"
    out = [b[16:-16].copy() if w else None for b, w in zip(bufs, want)]
    return (rc, out[0].view(capi.SHAPE_DTYPE), None if out[1] is None else out[1].view(np.uint32).reshape(85, 8), None if out[2] is None else out[2].view(np.uint16))


def test_header_python_mirror_and_exports():
    h = _header()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym, nargs in NEW.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m and len(strip(m.group(1)).split(",")) == nargs, sym
        assert sym in capi.SYMBOLS
    assert "fhevc_ctx" not in re.search(r"\bint\s+fhevc_pu_shape_select_merge\s*\(([^;]*)\);", h).group(1)
    for phrase in ("21 = the merge-candidate", "20 is not a slot", "Timed under slot 21", "Log2ParMrgLevel 2", "TEncSearch.cpp:2831-2884", "TComDataCU.cpp:2142-2320",
                   "19 = the merge-candidate costs", "18 is not a slot", "Timed under slot 19"):
        assert phrase in h, phrase
    sig = inspect.signature(capi.Context.motion_merge_pu)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "refined", "origin", "stride", "qp", "max_range", "with_pus", "with_small"]
    sig = inspect.signature(capi.Context.motion_merge_pu_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_refined", "d_out_pus", "d_out_pus_small", "rows", "stream",
                                    "qp", "max_range"]
    sig = inspect.signature(capi.Context.pu_shape_select_merge_device)
    assert list(sig.parameters) == ["self", "d_nodes", "d_pus", "d_pus_small", "d_merge_pus", "d_merge_pus_small", "num_pictures", "d_shapes", "d_costs", "d_merged", "rows",
                                    "stream", "rule"]
    assert hasattr(capi.Context, "p_tree_merge_pu_frame") and hasattr(capi, "pu_shape_select_merge")
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym


def test_rejected_without_a_device_and_the_timing_slots():
    lib = capi.load_library()
    assert lib.fhevc_motion_merge_pu_device(None, None, 2, 64, 0, 2, 0, 1, 32, 4, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_merge_pu(None, None, None, 64, 32, 4, None, None, None) == capi.E_INVALID
    assert lib.fhevc_pu_shape_select_merge_device(None, None, None, None, None, None, 1, 0, 1, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_p_tree_merge_pu_frame(None, None, None, 64, 32, 8, 0, None, None, None, None, None, None) == capi.E_INVALID
    for slot in (21, 20, 22):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # the host twin: what fhevc_pu_shape_select rejects, and a NULL merge_pus; merge_pus_small, costs and merged may be NULL
    rng = np.random.default_rng(5)
    nodes, pus, small = (a[0, 0] for a in sr.random_entries(rng, 1, 1))
    mpus, msmall = (a[0, 0] for a in mpr.random_pu_merge(rng, pus[None, None], small[None, None]))
    d = capi.pu_shape_rule_default()
    call = lambda **kw: host_select(kw.get("nodes", nodes), kw.get("pus", pus), kw.get("small", small), kw.get("mpus", mpus), kw.get("msmall", msmall), kw.get("vw", 64),
                                    kw.get("vh", 64), kw.get("rule", d), kw.get("want_costs", True), kw.get("want_merged", True))
    assert call()[0] == capi.OK
    for change in (dict(msmall=None), dict(small=None), dict(want_costs=False), dict(want_merged=False), dict(small=None, msmall=None, want_costs=False, want_merged=False)):
        assert call(**change)[0] == capi.OK, change
    for change in (dict(mpus=None), dict(nodes=None), dict(pus=None), dict(rule=None), dict(vw=7), dict(vh=65), dict(rule=capi.pu_shape_rule([0, 65536, 0, 0], [0] * 4, 1)),
                   dict(rule=capi.pu_shape_rule([0] * 4, [0, -1, 0, 0], 1)), dict(rule=capi.pu_shape_rule([0] * 4, [0] * 4, 2))):
        assert call(**change)[0] == capi.E_INVALID, change          # host_select asserts that nothing was written


def test_host_twin_equals_the_restatement_on_random_ctus():
    rng = np.random.default_rng(417)
    n = 96
    nodes, pus, small = sr.random_entries(rng, 1, n)
    mpus, msmall = mpr.random_pu_merge(rng, pus, small)
    seen = {l: set() for l in range(4)}
    bits = 0
    changed = 0
    for c in range(n):
        vw, vh = GEOMETRIES[c % 8]
        rule = sr.random_rule(rng, c % 2) if c % 3 else capi.pu_shape_rule_default()
        use_small, use_msmall = c % 5 != 4, c % 7 != 6
        args = (nodes[0, c], pus[0, c], small[0, c] if use_small else None, mpus[0, c], msmall[0, c] if use_msmall else None)
        rc, rec, costs, merged = host_select(*args, vw, vh, rule, want_costs=c % 4 != 3, want_merged=c % 6 != 5)
        assert rc == capi.OK
        sl = lambda a, use=True: a[:, c:c + 1] if use else None
        erec, ecosts, emerged = mpr.select(sl(nodes), sl(pus), sl(small, use_small), sl(mpus), sl(msmall, use_msmall), vw, vh, rule=rule)
        sr.same(rec, erec[0, 0], (c, vw, vh))
        if costs is not None:
            assert np.array_equal(costs, ecosts[0, 0]), (c, vw, vh)
        if merged is not None:
            assert np.array_equal(merged, emerged[0, 0]), (c, vw, vh, np.argwhere(merged != emerged[0, 0])[:5])
        bits += int(np.count_nonzero(emerged))
        plain = sr.select(sl(nodes), sl(pus), sl(small, use_small), vw, vh, rule=rule)[0]
        changed += int((plain["best"] != erec["best"]).sum())
        for l, s in mpr.part_combinations(sl(pus), sl(small), sl(mpus), sl(msmall), vw, vh).items():
            seen[l] |= s
    # (refined available, merge available) in all four combinations at every level; bits set and not set; the merge costs change decisions
    for l in range(4):
        assert seen[l] == {(True, True), (True, False), (False, True), (False, False)}, (l, seen[l])
    assert 0 < bits < n * 85 and changed > 0
    # all merge costs MARK: byte for byte fhevc_pu_shape_select, through the Python mirrors; random bytes elsewhere in the records
    W, H = 100, 76
    none_p, none_s = mpus[0, :4].copy(), msmall[0, :4].copy()
    none_p["cost_best"], none_s["cost_best"] = MARK, MARK
    rule = sr.random_rule(rng, 1)
    a = capi.pu_shape_select(nodes[0, :4], pus[0, :4], small[0, :4], W, H, rule, with_costs=True)
    for ms in (none_s, None):
        b = capi.pu_shape_select_merge(nodes[0, :4], pus[0, :4], small[0, :4], none_p, ms, W, H, rule, with_costs=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and not b[2].any()
    got = capi.pu_shape_select_merge(nodes[0, :4], pus[0, :4], small[0, :4], mpus[0, :4], msmall[0, :4], W, H, rule, with_costs=True)
    exp = mpr.select(nodes[:, :4], pus[:, :4], small[:, :4], mpus[:, :4], msmall[:, :4], W, H, rule=rule)
    sr.same(got[0], exp[0][0])
    assert np.array_equal(got[1], exp[1][0]) and np.array_equal(got[2], exp[2][0])
