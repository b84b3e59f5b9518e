"""The C-ABI surface of the partition-size selection and its host function (no GPU needed: the library loads without one for context-free
functions): fhevc_pu_shape_select against the numpy restatement of tests/pu_shape_ref.py on random CTUs drawn so that every case of the
definition occurs, fhevc_pu_shape_rule_default, the struct sizes, the header's constants and the Python mirror."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import pu_shape_ref as sr
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fhevc_pu_shape_rule_default", "fhevc_pu_shape_select", "fhevc_pu_shape_select_device", "fhevc_p_shape_frame")
SIZES = (64, 40, 8)


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def host_select(nodes, pus, small, vw, vh, rule, want_costs=True):
    """fhevc_pu_shape_select on one CTU -> (rc, records [85], costs [85, 8] or None); outputs pre-filled with a canary"""
    lib = capi.load_library()
    rec = np.full(85 * 16 + 32, 0xA5, np.uint8)
    costs = np.full(85 * 8 * 4 + 32, 0xA5, np.uint8)
    held = [None if a is None else np.ascontiguousarray(a) for a in (nodes, pus, small)]
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = lib.fhevc_pu_shape_select(ptr(held[0]), ptr(held[1]), ptr(held[2]), vw, vh, C.byref(rule) if rule is not None else None,
                                   rec.ctypes.data + 16, costs.ctypes.data + 16 if want_costs else None)
    assert (rec[:16] == 0xA5).all() and (rec[-16:] == 0xA5).all() and (costs[:16] == 0xA5).all() and (costs[-16:] == 0xA5).all()
    if not want_costs:
        assert (costs == 0xA5).all()
    return rc, rec[16:-16].copy().view(capi.SHAPE_DTYPE), costs[16:-16].copy().view(np.uint32).reshape(85, 8) if want_costs else None


@pytest.mark.parametrize("amp_mode", [0, 1])
def test_host_function_equals_the_restatement_on_random_ctus(amp_mode):
    rng = np.random.default_rng(300 + amp_mode)
    n = 48
    nodes, pus, small = (a[0] for a in sr.random_entries(rng, 1, n))
    seen = dict(tie=0, saturated=0, marker_2Nx2N=0, none=0, gated=0, second_none=0, invalid=0, levels=set())
    for c in range(n):
        vw, vh = SIZES[c % 3], SIZES[(c // 3) % 3]
        rule = sr.random_rule(rng, amp_mode) if c % 4 else capi.pu_shape_rule(0, 0, amp_mode)
        use_small = c % 5 != 4
        rc, rec, costs = host_select(nodes[c], pus[c], small[c] if use_small else None, vw, vh, rule, want_costs=c % 2 == 0)
        assert rc == capi.OK
        erec, ecosts = sr.select_ctu(nodes["cost_best"][c], pus["cost_best"][c], small["cost_best"][c] if use_small else None, vw, vh, rule)
        sr.same(rec, erec, (c, vw, vh))
        if costs is not None:
            assert np.array_equal(costs, ecosts), (c, np.argwhere(costs != ecosts)[:5])
        valid = erec["mask"] != 0
        seen["tie"] += int(((erec["cost_best"] == erec["cost_second"]) & (erec["best"] != 255)).sum())
        seen["saturated"] += int((ecosts == sr.SATURATED).sum())
        seen["marker_2Nx2N"] += int((valid & (erec["cost_2Nx2N"] == sr.MARKER)).sum())
        seen["none"] += int((valid & (erec["best"] == 255)).sum())
        seen["second_none"] += int((valid & (erec["best"] != 255) & (erec["second"] == 255)).sum())
        seen["gated"] += int((erec["avail"] & ~erec["mask"] & 0xF0 != 0).sum())
        seen["invalid"] += int((~valid).sum())
        seen["levels"] |= {sr.level(k) for k in np.flatnonzero(~valid)} if (vw, vh) != (8, 8) else set()
    # every case of the definition occurred in the draw (amp_mode 0 gates nothing: every AMP bit it clears is the margin's doing)
    assert seen["tie"] and seen["saturated"] and seen["marker_2Nx2N"] and seen["invalid"] and seen["levels"] == {0, 1, 2, 3}, seen
    assert seen["gated"], seen


def test_rule_default_and_rejected_arguments():
    lib = capi.load_library()
    r = capi.PuShapeRule((C.c_int32 * 4)(9, 9, 9, 9), (C.c_int32 * 4)(9, 9, 9, 9), 7)
    lib.fhevc_pu_shape_rule_default(C.byref(r))
    assert list(r.margin_q8) == [0, 0, 0, 0] and list(r.margin_abs) == [0, 0, 0, 0] and r.amp_mode == 1
    lib.fhevc_pu_shape_rule_default(None)      # tolerated, as fhevc_p_rule_default
    d = capi.pu_shape_rule_default()
    assert bytes(d) == bytes(r)
    rng = np.random.default_rng(9)
    nodes, pus, small = (a[0, 0] for a in sr.random_entries(rng, 1, 1))
    ok = lambda **kw: host_select(kw.get("nodes", nodes), kw.get("pus", pus), small, kw.get("vw", 64), kw.get("vh", 64), kw.get("rule", d))
    assert ok()[0] == capi.OK
    bad_rules = [capi.pu_shape_rule([0, 0, -1, 0], 0, 1), capi.pu_shape_rule([65536, 0, 0, 0], 0, 1), capi.pu_shape_rule(0, [0, 0, 0, -1], 1),
                 capi.pu_shape_rule(0, 0, 2), capi.pu_shape_rule(0, 0, -1)]
    for change in [dict(vw=0), dict(vw=65), dict(vh=7), dict(vh=72), dict(rule=None), dict(nodes=None), dict(pus=None)] + [dict(rule=b) for b in bad_rules]:
        rc, rec, costs = ok(**change)
        assert rc == capi.E_INVALID, change
        assert (rec.view(np.uint8) == 0xA5).all() and (costs.view(np.uint8) == 0xA5).all(), "a rejected call wrote"
    assert ok(rule=capi.pu_shape_rule(65535, 0x7FFFFFFF, 0))[0] == capi.OK
    assert lib.fhevc_pu_shape_select(nodes.ctypes.data, pus.ctypes.data, small.ctypes.data, 64, 64, C.byref(d), None, None) == capi.E_INVALID


def test_struct_sizes_and_constants():
    assert capi.SHAPE_DTYPE.itemsize == 16 and C.sizeof(capi.PuShapeRule) == 36
    assert [capi.SHAPE_DTYPE.fields[f][1] for f in ("cost_2Nx2N", "cost_best", "cost_second", "best", "second", "mask", "avail")] == [0, 4, 8, 12, 13, 14, 15]
    h = _header()
    values = {name: int(v) for name, v in re.findall(r"#define\s+FHEVC_PART_(\w+)\s+(\d+)", h)}
    # HM's PartSize (TypeDef.h): SIZE_2Nx2N, SIZE_2NxN, SIZE_Nx2N, SIZE_NxN, SIZE_2NxnU, SIZE_2NxnD, SIZE_nLx2N, SIZE_nRx2N = 0..7
    assert values == {"2Nx2N": 0, "2NxN": 1, "Nx2N": 2, "2NxnU": 4, "2NxnD": 5, "nLx2N": 6, "nRx2N": 7}
    assert (capi.PART_2Nx2N, capi.PART_2NxN, capi.PART_Nx2N, capi.PART_2NxnU, capi.PART_2NxnD, capi.PART_nLx2N, capi.PART_nRx2N) == (0, 1, 2, 4, 5, 6, 7)
    assert sr.ORDER == (0, 2, 1, 4, 5, 6, 7)
    rec = re.search(r"typedef struct \{([^}]*)\}\s*fhevc_pu_shape_node;", h).group(1)
    assert re.findall(r"(uint\d+_t)\s+([\w, ]+);", rec) == [("uint32_t", "cost_2Nx2N"), ("uint32_t", "cost_best"), ("uint32_t", "cost_second"),
                                                            ("uint8_t", "best, second"), ("uint8_t", "mask"), ("uint8_t", "avail")]
    rule = re.search(r"typedef struct \{([^}]*)\}\s*fhevc_pu_shape_rule;", h).group(1)
    assert re.findall(r"int32_t\s+(\w+)(\[4\])?;", rule) == [("margin_q8", "[4]"), ("margin_abs", "[4]"), ("amp_mode", "")]
    assert re.search(r"13 = the partition-size selection", h)


def test_header_python_mirror_and_exports():
    h = _header()
    dev = re.search(r"\bint\s+fhevc_pu_shape_select_device\s*\(([^;]*)\);", h).group(1)
    assert len(dev.split(",")) == 11 and dev.strip().startswith("fhevc_ctx*") and "const fhevc_pu_shape_rule* rule" in dev and dev.strip().endswith("void* stream")
    host = re.search(r"\bint\s+fhevc_pu_shape_select\s*\(([^;]*)\);", h).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", host).split(",")) == 8 and "fhevc_ctx" not in host
    frame = re.search(r"\bint\s+fhevc_p_shape_frame\s*\(([^;]*)\);", h).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", frame).split(",")) == 8
    for sym in NEW:
        assert sym in capi.SYMBOLS
    sig = inspect.signature(capi.Context.pu_shape_select_device)
    assert list(sig.parameters) == ["self", "d_nodes", "d_pus", "d_pus_small", "num_pictures", "d_shapes", "d_costs", "rows", "stream", "rule"]
    assert hasattr(capi.Context, "p_shape_frame")
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym in NEW:
        assert re.search(rf"\bT {sym}\b", exported), sym
    assert len(lib.fhevc_pu_shape_select_device.argtypes) == 11 and len(lib.fhevc_p_shape_frame.argtypes) == 8 and len(lib.fhevc_pu_shape_select.argtypes) == 8
    # without a context both device forms refuse before they touch a device
    assert lib.fhevc_pu_shape_select_device(None, None, None, None, 1, 0, 1, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_p_shape_frame(None, None, None, 64, 32, 8, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 13, 0, None, None) == capi.E_INVALID
