"""The C-ABI surface of the tree decision and its host function (no GPU needed: the library loads without one for context-free functions):
fhevc_p_tree_select against the Python restatement of tests/p_tree_ref.py on random CTUs drawn so that every case of the definition occurs at every
level, fhevc_p_tree_rule_default, the struct sizes, the header's signatures and the Python mirror."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import p_tree_ref as tr
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fhevc_p_tree_rule_default", "fhevc_p_tree_select", "fhevc_p_tree_select_device", "fhevc_p_tree_frame")
# three whole CTUs in eight (only they have a decision at level 0), the rest ragged on either or both sides
GEOMETRIES = [(64, 64), (64, 64), (64, 64), (40, 64), (64, 12), (36, 40), (8, 8), (12, 36)]
CANARY = 0xA5


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def host_select(shapes, vw, vh, rule, want=(True, True, True)):
    """fhevc_p_tree_select on one CTU -> (rc, depth_min [256], depth_max [256], records [85]), None for an output not asked for; every output lies between
    canaries, and one not asked for stays untouched"""
    lib = capi.load_library()
    sizes = (256, 256, 85 * 16)
    bufs = [np.full(n + 32, CANARY, np.uint8) for n in sizes]
    held = None if shapes is None else np.ascontiguousarray(shapes)
    rc = lib.fhevc_p_tree_select(None if held is None else held.ctypes.data, vw, vh, C.byref(rule) if rule is not None else None,
                                 *[b.ctypes.data + 16 if w else None for b, w in zip(bufs, want)])
    for b, w in zip(bufs, want):
        assert (b[:16] == CANARY).all() and (b[-16:] == CANARY).all(), "a canary around an output was written"
        if not w or rc != capi.OK:
            assert (b == CANARY).all(), "an output that was not asked for, or of a rejected call, was written"
    out = [b[16:-16].copy() if w else None for b, w in zip(bufs, want)]
    if out[2] is not None:
        out[2] = out[2].view(capi.TREE_DTYPE)
    return (rc, *out)


def test_host_function_equals_the_restatement_on_random_ctus():
    rng = np.random.default_rng(300)
    n = 96
    shapes = tr.random_shapes(rng, 1, n)[0]
    seen = None
    combos = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True), (True, False, True)]
    for c in range(n):
        vw, vh = GEOMETRIES[c % 8]
        rule = tr.random_rule(rng) if c % 3 else capi.p_tree_rule_default()
        want = combos[c % 7]
        rc, dmin, dmax, rec = host_select(shapes[c], vw, vh, rule, want)
        assert rc == capi.OK
        erec, emin, emax = tr.tree_ctu(shapes["cost_best"][c], vw, vh, rule)
        assert (emin <= emax).all()
        if dmin is not None:
            assert np.array_equal(dmin, emin), (c, vw, vh)
        if dmax is not None:
            assert np.array_equal(dmax, emax), (c, vw, vh)
        if rec is not None:
            tr.same(rec, erec, (c, vw, vh))
        seen = tr.coverage(erec, seen)
    # every case of the definition occurred in the draw at every level 0..2 (an ABSENT root cannot exist: node (0, 0) is never OUTSIDE)
    for case in tr.CASES:
        assert seen[case] == ({1, 2} if case == "absent" else {0, 1, 2}), (case, seen)
    assert tr.covers_everything(seen)


def test_rule_default_and_rejected_arguments():
    lib = capi.load_library()
    nine = lambda: (C.c_int32 * 3)(9, 9, 9)
    r = capi.PTreeRule(nine(), nine(), nine(), nine(), nine())
    lib.fhevc_p_tree_rule_default(C.byref(r))
    assert bytes(r) == bytes(60)
    lib.fhevc_p_tree_rule_default(None)      # tolerated, as fhevc_pu_shape_rule_default
    d = capi.p_tree_rule_default()
    assert bytes(d) == bytes(r)
    rng = np.random.default_rng(9)
    shapes = tr.random_shapes(rng, 1, 1)[0, 0]
    ok = lambda **kw: host_select(kw.get("shapes", shapes), kw.get("vw", 64), kw.get("vh", 64), kw.get("rule", d), kw.get("want", (True, True, True)))
    assert ok()[0] == capi.OK
    mk = capi.p_tree_rule
    bad_rules = [mk(split_q8=[0, -1, 0]), mk(split_q8=[65536, 0, 0]), mk(stop_q8=[0, 0, -1]), mk(stop_q8=[0, 65536, 0]), mk(split_abs=[0, 0, -1]),
                 mk(stop_abs=[-1, 0, 0]), mk(split_cost=[0, -1, 0])]
    for change in [dict(vw=0), dict(vw=7), dict(vw=65), dict(vh=7), dict(vh=72), dict(rule=None), dict(shapes=None), dict(want=(False, False, False))] + \
                  [dict(rule=b) for b in bad_rules]:
        assert ok(**change)[0] == capi.E_INVALID, change          # host_select asserts that nothing was written
    assert ok(rule=mk(65535, 0x7FFFFFFF, 65535, 0x7FFFFFFF, 0x7FFFFFFF))[0] == capi.OK


def test_struct_sizes_and_offsets():
    assert C.sizeof(capi.PTreeRule) == 60 and capi.TREE_DTYPE.itemsize == 16
    assert [getattr(capi.PTreeRule, f).offset for f in ("split_q8", "split_abs", "stop_q8", "stop_abs", "split_cost")] == [0, 12, 24, 36, 48]
    assert [capi.TREE_DTYPE.fields[f][1] for f in ("cost_own", "cost_kids", "cost_tree", "flags", "level", "pad")] == [0, 4, 8, 12, 13, 14]
    h = _header()
    rec = re.search(r"typedef struct \{([^}]*)\}\s*fhevc_p_tree_node;", h).group(1)
    assert re.findall(r"(uint\d+_t)\s+([\w\[\]]+);", rec) == [("uint32_t", "cost_own"), ("uint32_t", "cost_kids"), ("uint32_t", "cost_tree"), ("uint8_t", "flags"),
                                                              ("uint8_t", "level"), ("uint8_t", "pad[2]")]
    rule = re.search(r"typedef struct \{([^}]*)\}\s*fhevc_p_tree_rule;", h).group(1)
    assert re.findall(r"int32_t\s+(\w+)\[3\];", rule) == ["split_q8", "split_abs", "stop_q8", "stop_abs", "split_cost"]
    # the library writes the record as the header lays it out
    _, _, _, got = host_select(np.zeros(85, capi.SHAPE_DTYPE), 64, 64, capi.p_tree_rule_default())
    assert got["level"].tolist() == [0] + [1] * 4 + [2] * 16 + [3] * 64 and (got["pad"] == 0).all() and (got["cost_own"] == 0).all()
    assert (got["cost_kids"][21:] == tr.MARK).all() and (got["flags"][:21] == tr.STOP_SURE | tr.OWN_AVAILABLE | tr.KIDS_AVAILABLE).all()


def test_header_python_mirror_and_exports():
    h = _header()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = strip(re.search(r"\bint\s+fhevc_p_tree_select_device\s*\(([^;]*)\);", h).group(1))
    assert len(dev.split(",")) == 10 and dev.strip().startswith("fhevc_ctx*") and "const fhevc_p_tree_rule* rule" in dev and dev.strip().endswith("void* stream")
    host = strip(re.search(r"\bint\s+fhevc_p_tree_select\s*\(([^;]*)\);", h).group(1))
    assert len(host.split(",")) == 7 and "fhevc_ctx" not in host
    frame = strip(re.search(r"\bint\s+fhevc_p_tree_frame\s*\(([^;]*)\);", h).group(1))
    assert len(frame.split(",")) == 12 and "int coarse_range" in frame
    assert "17 = the P-picture tree decision" in h and "16 is not a slot" in h and "Timed under slot 17" in h
    assert h.count("fhevc_p_tree_frame, further below") == 2          # behind the "NOT covered" lines of the two centred entry points
    for sym in NEW:
        assert sym in capi.SYMBOLS
    for name in ("PTreeRule", "TREE_DTYPE", "p_tree_rule", "p_tree_rule_default"):
        assert hasattr(capi, name), name
    sig = inspect.signature(capi.Context.p_tree_select_device)
    assert list(sig.parameters) == ["self", "d_shapes", "num_pictures", "d_depth_min", "d_depth_max", "d_tree", "rows", "stream", "rule"]
    assert hasattr(capi.Context, "p_tree_frame")
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym in NEW:
        assert re.search(rf"\bT {sym}\b", exported), sym
    assert len(lib.fhevc_p_tree_select_device.argtypes) == 10 and len(lib.fhevc_p_tree_frame.argtypes) == 12 and len(lib.fhevc_p_tree_select.argtypes) == 7
    # without a context both device forms refuse before they touch a device
    assert lib.fhevc_p_tree_select_device(None, None, 1, 0, 1, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_p_tree_frame(None, None, None, 64, 32, 8, 0, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 17, 0, None, None) == capi.E_INVALID


def test_python_mirror_of_the_host_function():
    rng = np.random.default_rng(12)
    W, H = 100, 76
    shapes = tr.random_shapes(rng, 1, 4)[0]
    rule = tr.random_rule(rng)
    erec, emin, emax = tr.select(shapes[None], W, H, rule=rule)
    dmin, dmax, rec = capi.p_tree_select(shapes, W, H, rule, with_tree=True)
    tr.same(rec, erec[0])
    assert np.array_equal(dmin, emin[0]) and np.array_equal(dmax, emax[0])
    lo, hi = capi.p_tree_select(shapes, W, H)
    elo = tr.select(shapes[None], W, H)
    assert np.array_equal(lo, elo[1][0]) and np.array_equal(hi, elo[2][0])
    assert bytes(capi.p_tree_rule(1, [2, 3, 4], 5, 6, [7, 8, 9])) == np.array([1, 1, 1, 2, 3, 4, 5, 5, 5, 6, 6, 6, 7, 8, 9], np.int32).tobytes()
