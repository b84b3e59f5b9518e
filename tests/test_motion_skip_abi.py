"""The C-ABI surface of the zero-residual stage and of the tree decision that stops at a skip (no GPU needed: the library loads without one for
context-free functions): the 16-byte fhevc_motion_skip_node in the header and in the Python mirror, the four entry points' signatures and exports, calls
rejected before a device is touched, fhevc_p_tree_select_skip against the Python restatement of tests/motion_skip_ref.py on random CTUs, timing slots
22, 23 and 24."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import numpy as np

import motion_merge_ref as mg
import motion_skip_ref as sk
import p_tree_ref as tr
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_motion_skip_device": 13, "fhevc_motion_skip": 8, "fhevc_p_tree_select_skip": 10, "fhevc_p_tree_select_skip_device": 13}
GEOMETRIES = [(64, 64), (64, 64), (64, 64), (40, 64), (64, 12), (36, 40), (8, 8), (12, 36)]
CANARY = 0xA5


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def host_select(shapes, merge, skip, mask, vw, vh, rule, want=(True, True, True)):
    """fhevc_p_tree_select_skip on one CTU -> (rc, depth_min, depth_max, records), None for an output not asked for; outputs between canaries"""
    lib = capi.load_library()
    bufs = [np.full(n + 32, CANARY, np.uint8) for n in (256, 256, 85 * 16)]
    ins = [None if a is None else np.ascontiguousarray(a) for a in (shapes, merge, skip)]
    ptr = [None if a is None else a.ctypes.data for a in ins]
    rc = lib.fhevc_p_tree_select_skip(ptr[0], ptr[1], ptr[2], mask, vw, vh, C.byref(rule) if rule is not None else None,
                                      *[b.ctypes.data + 16 if w else None for b, w in zip(bufs, want)])
    for b, w in zip(bufs, want):
        assert (b[:16] == CANARY).all() and (b[-16:] == CANARY).all(), "a canary around an output was written"
        if not w or rc != capi.OK:
            assert (b == CANARY).all(), "an output that was not asked for, or of a rejected call, was written"
    out = [b[16:-16].copy() if w else None for b, w in zip(bufs, want)]
    if out[2] is not None:
        out[2] = out[2].view(capi.TREE_DTYPE)
    return (rc, *out)


def test_struct_size_and_offsets():
    d = capi.MOTION_SKIP_DTYPE
    assert d.itemsize == 16 and d.names == ("coef_max", "level_sum", "nonzero", "flags", "pad", "mvx", "mvy")
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 10, 11, 12, 14]
    assert [d.fields[n][0].str for n in d.names] == ["<u4", "<u4", "<u2", "|u1", "|u1", "<i2", "<i2"]
    assert (capi.SKIP_ZERO_PLAIN, capi.SKIP_ZERO_HALF) == (1, 2) == (sk.ZERO_PLAIN, sk.ZERO_HALF)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fhevc_motion_skip_node\s*;", _header())
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t coef_max", "uint32_t level_sum", "uint16_t nonzero", "uint8_t flags", "uint8_t pad", "int16_t mvx, mvy"]
    # the record's size is pinned where it is compiled, too
    assert "static_assert(sizeof(FhevcMotionSkipNode) == 16" in open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_internal.h")).read()


def test_header_python_mirror_and_exports():
    h = _header()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym, nargs in NEW.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m and len(strip(m.group(1)).split(",")) == nargs, sym
        assert sym in capi.SYMBOLS
    assert "fhevc_ctx" not in re.search(r"\bint\s+fhevc_p_tree_select_skip\s*\(([^;]*)\);", h).group(1)
    for phrase in ("23 = the zero-residual test", "22 is not a slot", "Timed under slot 23", "TEncCu.cpp:892", ":610-637", ":1444-1468", "TComTrQuant.cpp:860-915",
                   "TComTrQuant.cpp:1186-1232", "cfg/encoder_lowdelay_P_main.cfg:12", ":1215", ":2257", ":2264", "{26214, 23302, 20560, 18396, 16384, 14564}",
                   "20 is not a slot", "18 is not a slot", "16 is not a slot"):
        assert phrase in h, phrase
    sig = inspect.signature(capi.Context.motion_skip)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "merge", "origin", "stride", "qp", "max_range"]
    sig = inspect.signature(capi.Context.motion_skip_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_merge", "d_out", "rows", "stream", "qp", "max_range"]
    sig = inspect.signature(capi.Context.p_tree_select_skip_device)
    assert list(sig.parameters) == ["self", "d_shapes", "d_merge", "d_skip", "skip_mask", "num_pictures", "d_depth_min", "d_depth_max", "d_tree", "rows", "stream", "rule"]
    assert hasattr(capi, "p_tree_select_skip")
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym


def test_rejected_without_a_device_and_the_timing_slots():
    lib = capi.load_library()
    assert lib.fhevc_motion_skip_device(None, None, 2, 64, 0, 2, 0, 1, 32, 4, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_skip(None, None, None, 64, 32, 4, None, None) == capi.E_INVALID
    assert lib.fhevc_p_tree_select_skip_device(None, None, None, None, 1, 1, 0, 1, None, None, None, None, None) == capi.E_INVALID
    for slot in (22, 23, 24):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # the host twin: what fhevc_p_tree_select_merge rejects, a NULL skip pointer, skip_mask outside 0..3
    rng = np.random.default_rng(5)
    shapes = tr.random_shapes(rng, 1, 1)
    merge = mg.random_merge(rng, shapes)
    skip = sk.random_skip(rng, (1, 1, 85))
    d = capi.p_tree_rule_default()
    ok = lambda **kw: host_select(kw.get("shapes", shapes[0, 0]), kw.get("merge", merge[0, 0]), kw.get("skip", skip[0, 0]), kw.get("mask", 3), kw.get("vw", 64),
                                  kw.get("vh", 64), kw.get("rule", d), kw.get("want", (True, True, True)))
    assert ok()[0] == capi.OK
    for change in (dict(skip=None), dict(mask=-1), dict(mask=4), dict(merge=None), dict(shapes=None), dict(rule=None), dict(vw=7), dict(vh=65),
                   dict(want=(False, False, False)), dict(rule=capi.p_tree_rule(split_q8=[0, 65536, 0])), dict(rule=capi.p_tree_rule(split_cost=[-1, 0, 0]))):
        assert ok(**change)[0] == capi.E_INVALID, change          # host_select asserts that nothing was written


def test_host_twin_equals_the_restatement_on_random_ctus():
    rng = np.random.default_rng(302)
    n = 96
    shapes = tr.random_shapes(rng, 1, n)
    merge = mg.random_merge(rng, shapes)
    skip = sk.random_skip(rng, (1, n, 85))
    combos = [w for w in itertools.product((True, False), repeat=3) if any(w)]
    assert len(combos) == 7
    seen_tree = None
    skipped = {l: 0 for l in range(3)}
    for c in range(n):
        vw, vh = GEOMETRIES[c % 8]
        rule = tr.random_rule(rng) if c % 3 else capi.p_tree_rule_default()
        for mask in range(4):
            erec, emin, emax = (a[0, 0] for a in sk.tree_select(shapes[:, c:c + 1], merge[:, c:c + 1], skip[:, c:c + 1], mask, vw, vh, rule=rule))
            for want in (combos if mask == c % 4 else [combos[(c + mask) % 7]]):
                rc, dmin, dmax, rec = host_select(shapes[0, c], merge[0, c], skip[0, c], mask, vw, vh, rule, want)
                assert rc == capi.OK
                if dmin is not None:
                    assert np.array_equal(dmin, emin), (c, mask, vw, vh)
                if dmax is not None:
                    assert np.array_equal(dmax, emax), (c, mask, vw, vh)
                if rec is not None:
                    tr.same(rec, erec, (c, mask, vw, vh))
            if mask == 3:
                seen_tree = tr.coverage(erec, seen_tree)
                for k in np.flatnonzero(erec["flags"] & sk.SKIPPED):
                    skipped[tr.level(k)] += 1
            if mask == 0:      # byte for byte the merge tree's host form
                base = mg.tree_select(shapes[:, c:c + 1], merge[:, c:c + 1], vw, vh, rule=rule)
                assert erec.tobytes() == base[0][0, 0].tobytes() and np.array_equal(emin, base[1][0, 0]) and np.array_equal(emax, base[2][0, 0])
    assert all(v > 0 for v in skipped.values()), skipped
    assert all(seen_tree[case] == {0, 1, 2} for case in ("split_sure", "stop_sure", "crossing")), seen_tree
    # records off their natural 16-byte alignment (any 4-byte alignment is allowed): the same bytes
    raw = np.zeros(85 * 16 + 16, np.uint8)
    raw[4:4 + 85 * 16] = skip[0, 0].view(np.uint8).reshape(-1)
    shifted = raw[4:4 + 85 * 16].view(capi.MOTION_SKIP_DTYPE)
    assert shifted.ctypes.data % 16 != 0 or raw.ctypes.data % 16 != 0
    a = host_select(shapes[0, 0], merge[0, 0], skip[0, 0], 3, 64, 64, capi.p_tree_rule_default())
    b = host_select(shapes[0, 0], merge[0, 0], shifted, 3, 64, 64, capi.p_tree_rule_default())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    # through the Python mirror, a ragged picture
    W, H = 100, 76
    rule = tr.random_rule(rng)
    got = capi.p_tree_select_skip(shapes[0, :4], merge[0, :4], skip[0, :4], 2, W, H, rule, with_tree=True)
    exp = sk.tree_select(shapes[:, :4], merge[:, :4], skip[:, :4], 2, W, H, rule=rule)
    tr.same(got[2], exp[0][0])
    assert np.array_equal(got[0], exp[1][0]) and np.array_equal(got[1], exp[2][0])
