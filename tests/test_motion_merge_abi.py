"""The C-ABI surface of the merge stage and of the tree decision that takes its costs (no GPU needed: the library loads without one for context-free
functions): the 16-byte fhevc_motion_merge_node in the header and in the Python mirror, the five entry points' signatures and exports, calls rejected
before a device is touched, fhevc_p_tree_select_merge against the Python restatement of tests/motion_merge_ref.py on random CTUs, timing slots 19 and 18."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import motion_merge_ref as mg
import p_tree_ref as tr
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_motion_merge_device": 13, "fhevc_motion_merge": 8, "fhevc_p_tree_select_merge": 8, "fhevc_p_tree_select_merge_device": 11, "fhevc_p_tree_merge_frame": 13}
GEOMETRIES = [(64, 64), (64, 64), (64, 64), (40, 64), (64, 12), (36, 40), (8, 8), (12, 36)]
CANARY = 0xA5


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def host_select(shapes, merge, vw, vh, rule, want=(True, True, True)):
    """fhevc_p_tree_select_merge on one CTU -> (rc, depth_min, depth_max, records), None for an output not asked for; outputs between canaries"""
    lib = capi.load_library()
    bufs = [np.full(n + 32, CANARY, np.uint8) for n in (256, 256, 85 * 16)]
    sh = None if shapes is None else np.ascontiguousarray(shapes)
    me = None if merge is None else np.ascontiguousarray(merge)
    rc = lib.fhevc_p_tree_select_merge(None if sh is None else sh.ctypes.data, None if me is None else me.ctypes.data, vw, vh,
                                       C.byref(rule) if rule is not None else None, *[b.ctypes.data + 16 if w else None for b, w in zip(bufs, want)])
    for b, w in zip(bufs, want):
        assert (b[:16] == CANARY).all() and (b[-16:] == CANARY).all(), "a canary around an output was written"
        if not w or rc != capi.OK:
            assert (b == CANARY).all(), "an output that was not asked for, or of a rejected call, was written"
    out = [b[16:-16].copy() if w else None for b, w in zip(bufs, want)]
    if out[2] is not None:
        out[2] = out[2].view(capi.TREE_DTYPE)
    return (rc, *out)


def test_struct_size_and_offsets():
    d = capi.MOTION_MERGE_DTYPE
    assert d.itemsize == 16 and d.names == ("satd_best", "cost_best", "mvx", "mvy", "idx", "num", "src", "pad")
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 10, 12, 13, 14, 15]
    assert [d.fields[n][0].str for n in d.names] == ["<u4", "<u4", "<i2", "<i2", "|u1", "|u1", "|u1", "|u1"]
    # cost_best sits in dword 1, where the tree kernel reads it from the selection's records too
    assert capi.SHAPE_DTYPE.fields["cost_best"][1] == 4
    assert (capi.MERGE_L, capi.MERGE_A, capi.MERGE_AR, capi.MERGE_BL, capi.MERGE_AL, capi.MERGE_ZERO) == (0, 1, 2, 3, 4, 5)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fhevc_motion_merge_node\s*;", _header())
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t satd_best", "uint32_t cost_best", "int16_t mvx, mvy", "uint8_t idx", "uint8_t num", "uint8_t src", "uint8_t pad"]


def test_header_python_mirror_and_exports():
    h = _header()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym, nargs in NEW.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m and len(strip(m.group(1)).split(",")) == nargs, sym
        assert sym in capi.SYMBOLS
    assert "fhevc_ctx" not in re.search(r"\bint\s+fhevc_p_tree_select_merge\s*\(([^;]*)\);", h).group(1)
    assert "19 = the merge-candidate costs" in h and "18 is not a slot" in h and "Timed under slot 19" in h and "selectMotionLambda" in h
    sig = inspect.signature(capi.Context.motion_merge)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "refined", "origin", "stride", "qp", "max_range"]
    sig = inspect.signature(capi.Context.motion_merge_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_refined", "d_out", "rows", "stream", "qp", "max_range"]
    sig = inspect.signature(capi.Context.p_tree_select_merge_device)
    assert list(sig.parameters) == ["self", "d_shapes", "d_merge", "num_pictures", "d_depth_min", "d_depth_max", "d_tree", "rows", "stream", "rule"]
    assert hasattr(capi.Context, "p_tree_merge_frame") and hasattr(capi, "p_tree_select_merge")
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym


def test_rejected_without_a_device_and_the_timing_slots():
    lib = capi.load_library()
    assert lib.fhevc_motion_merge_device(None, None, 2, 64, 0, 2, 0, 1, 32, 4, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_merge(None, None, None, 64, 32, 4, None, None) == capi.E_INVALID
    assert lib.fhevc_p_tree_select_merge_device(None, None, None, 1, 0, 1, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_p_tree_merge_frame(None, None, None, 64, 32, 8, 0, None, None, None, None, None, None) == capi.E_INVALID
    for slot in (19, 18, 20):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # the host twin: what fhevc_p_tree_select rejects, and a NULL merge
    rng = np.random.default_rng(5)
    shapes = tr.random_shapes(rng, 1, 1)
    merge = mg.random_merge(rng, shapes)
    d = capi.p_tree_rule_default()
    ok = lambda **kw: host_select(kw.get("shapes", shapes[0, 0]), kw.get("merge", merge[0, 0]), kw.get("vw", 64), kw.get("vh", 64), kw.get("rule", d),
                                  kw.get("want", (True, True, True)))
    assert ok()[0] == capi.OK
    for change in (dict(merge=None), dict(shapes=None), dict(rule=None), dict(vw=7), dict(vh=65), dict(want=(False, False, False)),
                   dict(rule=capi.p_tree_rule(split_q8=[0, 65536, 0])), dict(rule=capi.p_tree_rule(split_cost=[-1, 0, 0]))):
        assert ok(**change)[0] == capi.E_INVALID, change          # host_select asserts that nothing was written


def test_host_twin_equals_the_restatement_on_random_ctus():
    rng = np.random.default_rng(301)
    n = 96
    shapes = tr.random_shapes(rng, 1, n)
    merge = mg.random_merge(rng, shapes)
    combos = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True), (True, False, True)]
    seen_tree = None
    seen = {l: set() for l in range(4)}
    bit6 = 0
    for c in range(n):
        vw, vh = GEOMETRIES[c % 8]
        rule = tr.random_rule(rng) if c % 3 else capi.p_tree_rule_default()
        rc, dmin, dmax, rec = host_select(shapes[0, c], merge[0, c], vw, vh, rule, combos[c % 7])
        assert rc == capi.OK
        # the restatement on a one-CTU picture of the CTU's valid size
        erec, emin, emax = (a[0, 0] for a in mg.tree_select(shapes[:, c:c + 1], merge[:, c:c + 1], vw, vh, rule=rule))
        if dmin is not None:
            assert np.array_equal(dmin, emin), (c, vw, vh)
        if dmax is not None:
            assert np.array_equal(dmax, emax), (c, vw, vh)
        if rec is not None:
            tr.same(rec, erec, (c, vw, vh))
        seen_tree = tr.coverage(erec, seen_tree)
        bit6 += int((erec["flags"] & mg.MERGED != 0).sum())
        for l, s in mg.availability_combinations(shapes[:, c:c + 1], merge[:, c:c + 1], vw, vh).items():
            seen[l] |= s
    # all four availability combinations occurred at every level, bit 6 both ways, and both decisions still occur at every level
    for l in range(4):
        assert seen[l] == {(True, True), (True, False), (False, True), (False, False)}, (l, seen[l])
    assert 0 < bit6 < n * 85 and all(seen_tree[case] == {0, 1, 2} for case in ("split_sure", "stop_sure", "crossing")), seen_tree
    # all merge costs MARK: byte for byte fhevc_p_tree_select, through the Python mirrors
    W, H = 100, 76
    none = np.zeros((4, 85), capi.MOTION_MERGE_DTYPE)
    none["cost_best"] = mg.MARK
    rule = tr.random_rule(rng)
    a = capi.p_tree_select(shapes[0, :4], W, H, rule, with_tree=True)
    b = capi.p_tree_select_merge(shapes[0, :4], none, W, H, rule, with_tree=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    got = capi.p_tree_select_merge(shapes[0, :4], merge[0, :4], W, H, rule, with_tree=True)
    exp = mg.tree_select(shapes[:, :4], merge[:, :4], W, H, rule=rule)
    tr.same(got[2], exp[0][0])
    assert np.array_equal(got[0], exp[1][0]) and np.array_equal(got[1], exp[2][0])
