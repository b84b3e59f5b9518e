"""The C-ABI surface of the RD stage and of the tree on RD costs (no GPU needed: the library loads without one for context-free functions): the 16-byte
fhevc_motion_rd_node in the header and in the Python mirror with dword 1 and byte 10 where the existing tree kernels read, the entry points' signatures
and exports, the header's normative phrases, lam_q8 of every QP, fhevc_p_tree_select_rd against fhevc_p_tree_select_skip on the same bytes and against
the restatement, rejected calls that write nothing, timing slots 28, 29 and 30."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import motion_rd_ref as rd
import motion_skip_ref as sk
import p_tree_ref as tr
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_motion_rd_device": 15, "fhevc_motion_rd": 10, "fhevc_p_tree_select_rd": 9, "fhevc_p_tree_select_rd_device": 12}
GEOMETRIES = [(64, 64), (64, 64), (40, 64), (64, 12), (36, 40), (8, 8)]
CANARY = 0xA5


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def random_rd(rng, shape):
    """RD records of random bytes with costs in the range where sums stay below the saturation, one in seven marked, flags of every value"""
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), capi.MOTION_RD_DTYPE).reshape(shape).copy()
    a["cost_rd"] = np.where(rng.random(shape) < 1 / 7, rd.MARK, a["cost_rd"] % 100000)
    return a


def host_tree(fn, ptrs, mask, vw, vh, rule, want=(True, True, True)):
    """fn = the RD tree (two record pointers) or the skip tree (three) on one CTU -> (rc, depth_min, depth_max, records); outputs between canaries"""
    bufs = [np.full(n + 32, CANARY, np.uint8) for n in (256, 256, 85 * 16)]
    rc = fn(*ptrs, mask, vw, vh, C.byref(rule) if rule is not None else None, *[b.ctypes.data + 16 if w else None for b, w in zip(bufs, want)])
    for b, w in zip(bufs, want):
        assert (b[:16] == CANARY).all() and (b[-16:] == CANARY).all(), "a canary around an output was written"
        if not w or rc != capi.OK:
            assert (b == CANARY).all(), "an output that was not asked for, or of a rejected call, was written"
    return (rc, *[b[16:-16].copy() if w else None for b, w in zip(bufs, want)])


def test_struct_size_and_offsets():
    d = capi.MOTION_RD_DTYPE
    assert d.itemsize == 16 and d.names == ("dist", "cost_rd", "bits", "flags", "tu_split", "mvx", "mvy")
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 10, 11, 12, 14]
    assert [d.fields[n][0].str for n in d.names] == ["<u4", "<u4", "<u2", "|u1", "|u1", "<i2", "<i2"]
    # dword 1 is where the selection and the merge records keep cost_best, byte 10 where the skip record keeps flags
    assert d.fields["cost_rd"][1] == capi.SHAPE_DTYPE.fields["cost_best"][1] == capi.MOTION_MERGE_DTYPE.fields["cost_best"][1] == 4
    assert d.fields["flags"][1] == capi.MOTION_SKIP_DTYPE.fields["flags"][1] == 10
    assert (capi.RD_SOURCE_MERGE, capi.RD_SOURCE_EXPLICIT, capi.RD_TU_SPLIT) == (0, 1, 4) and (rd.ZERO_PLAIN, rd.ZERO_HALF) == (capi.SKIP_ZERO_PLAIN, capi.SKIP_ZERO_HALF)
    h = _header()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fhevc_motion_rd_node\s*;", h)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t dist", "uint32_t cost_rd", "uint16_t bits", "uint8_t flags", "uint8_t tu_split", "int16_t mvx, mvy"]
    assert re.search(r"#define\s+FHEVC_RD_SOURCE_MERGE\s+0\b", h) and re.search(r"#define\s+FHEVC_RD_SOURCE_EXPLICIT\s+1\b", h)
    # the record's size and the two offsets are pinned where they are compiled, too
    assert "static_assert(sizeof(FhevcMotionRdNode) == 16" in open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_internal.h")).read()
    api = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_motion_api.hip")).read()
    assert "offsetof(fhevc_motion_rd_node, cost_rd) == 4 && offsetof(fhevc_motion_rd_node, flags) == 10" in api


def test_header_python_mirror_and_exports():
    h = _header()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym, nargs in NEW.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m and len(strip(m.group(1)).split(",")) == nargs, sym
        assert sym in capi.SYMBOLS
    assert "fhevc_ctx" not in re.search(r"\bint\s+fhevc_p_tree_select_rd\s*\(([^;]*)\);", h).group(1)
    for phrase in ("29 = the RD estimate", "28 is not a slot", "Timed under slot 29", "TComTrQuant.cpp:860-915", "TComTrQuant.cpp:1186-1232", "TComTrQuant.cpp:1387-1422",
                   "TComTrQuant.cpp:927-990", "TComRdCost.cpp:1190-1199", "TEncSearch.cpp:5117", "encodeResAndCalcRdInterCU", "xEstimateInterResidualQT",
                   "{40, 45, 51, 57, 64, 72}", "QuadtreeTUMaxDepthInter 3", "a third depth, which is left out", "RDOQ is NOT modelled", "the library's OWN estimate",
                   "0.57 * 2^((qp - 12) / 3)", "uiCbfAny && dSubdivCost < dSingleCost", "two of the seven partition sizes", "an expectation, not a", "inter 4x4 never takes the DST",
                   "targetInputBitDepth is 16"):
        assert phrase in h, phrase
    sig = inspect.signature(capi.Context.motion_rd)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "records", "source", "mvp", "origin", "stride", "qp", "max_range"]
    sig = inspect.signature(capi.Context.motion_rd_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "source", "d_in", "d_out", "d_mvp", "rows", "stream", "qp",
                                    "max_range"]
    sig = inspect.signature(capi.Context.p_tree_select_rd_device)
    assert list(sig.parameters) == ["self", "d_rd_explicit", "d_rd_merge", "skip_mask", "num_pictures", "d_depth_min", "d_depth_max", "d_tree", "rows", "stream", "rule"]
    assert hasattr(capi, "p_tree_select_rd")
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    assert re.search(r"\bT fhevc_motion_rd_lambda_q8\b", exported)
    # the new source is in the build list
    from fasthevc_amd import build
    assert "k_motion_rd.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "k_motion_rd.hip"))


def test_lambda_q8_of_every_qp_is_the_formula():
    lib = capi.load_library()
    assert [lib.fhevc_motion_rd_lambda_q8(qp) for qp in range(52)] == [rd.lam_q8(qp) for qp in range(52)]
    assert lib.fhevc_motion_rd_lambda_q8(-3) == rd.lam_q8(0) and lib.fhevc_motion_rd_lambda_q8(60) == rd.lam_q8(51)


def test_rejected_without_a_device_and_the_timing_slots():
    lib = capi.load_library()
    out = np.full(85 * 16, CANARY, np.uint8)
    rec = np.zeros(85, capi.MOTION_MERGE_DTYPE)
    pic = np.zeros((64, 64), np.int16)
    assert lib.fhevc_motion_rd_device(None, pic.ctypes.data, 2, 64, 4096, 2, 0, 1, 32, 4, 0, rec.ctypes.data, None, out.ctypes.data, None) == capi.E_INVALID
    assert lib.fhevc_motion_rd(None, pic.ctypes.data, pic.ctypes.data, 64, 32, 4, 0, rec.ctypes.data, None, out.ctypes.data) == capi.E_INVALID
    assert lib.fhevc_p_tree_select_rd_device(None, rec.ctypes.data, rec.ctypes.data, 1, 1, 0, 1, None, out.ctypes.data, None, None, None) == capi.E_INVALID
    assert (out == CANARY).all()
    for slot in (28, 29, 30):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # the host form of the tree: what fhevc_p_tree_select_skip rejects
    rng = np.random.default_rng(5)
    a, b = random_rd(rng, (85,)), random_rd(rng, (85,))
    d = capi.p_tree_rule_default()
    call = lambda **kw: host_tree(lib.fhevc_p_tree_select_rd, (kw.get("a", a.ctypes.data), kw.get("b", b.ctypes.data)), kw.get("mask", 3), kw.get("vw", 64), kw.get("vh", 64),
                                  kw.get("rule", d), kw.get("want", (True, True, True)))
    assert call()[0] == capi.OK
    for change in (dict(a=None), dict(b=None), dict(mask=-1), dict(mask=4), dict(rule=None), dict(vw=7), dict(vh=65), dict(want=(False, False, False)),
                   dict(rule=capi.p_tree_rule(split_q8=[0, 65536, 0])), dict(rule=capi.p_tree_rule(split_cost=[-1, 0, 0]))):
        assert call(**change)[0] == capi.E_INVALID, change            # host_tree asserts that nothing was written


def test_the_rd_tree_is_the_skip_tree_on_the_same_bytes_and_equals_the_restatement():
    lib = capi.load_library()
    rng = np.random.default_rng(411)
    n = 48
    a, b = random_rd(rng, (1, n, 85)), random_rd(rng, (1, n, 85))
    skipped = 0
    for c in range(n):
        vw, vh = GEOMETRIES[c % len(GEOMETRIES)]
        rule = tr.random_rule(rng) if c % 3 else capi.p_tree_rule_default()
        for mask in range(4):
            got = host_tree(lib.fhevc_p_tree_select_rd, (a[0, c].ctypes.data, b[0, c].ctypes.data), mask, vw, vh, rule)
            # ... the existing entry point on the records reinterpreted: b twice, as the merge records and as the skip records
            base = host_tree(lib.fhevc_p_tree_select_skip, (a[0, c].ctypes.data, b[0, c].ctypes.data, b[0, c].ctypes.data), mask, vw, vh, rule)
            assert got[0] == base[0] == capi.OK and all(x.tobytes() == y.tobytes() for x, y in zip(got[1:], base[1:])), (c, mask)
            erec, emin, emax = (x[0, 0] for x in rd.tree_select(a[:, c:c + 1], b[:, c:c + 1], mask, vw, vh, rule=rule))
            tr.same(got[3].view(capi.TREE_DTYPE), erec, (c, mask))
            assert np.array_equal(got[1], emin) and np.array_equal(got[2], emax)
            skipped += int(((erec["flags"] & sk.SKIPPED) != 0).sum())
    assert skipped > 0
    # bit 2 of flags (some TU split) is no bit of any mask: the tree does not see it
    c2 = b.copy()
    c2["flags"] ^= rd.TU_SPLIT
    c2["tu_split"] ^= 0xF
    c2["dist"] ^= 0x55
    x = host_tree(lib.fhevc_p_tree_select_rd, (a[0, 0].ctypes.data, b[0, 0].ctypes.data), 3, 64, 64, capi.p_tree_rule_default())
    y = host_tree(lib.fhevc_p_tree_select_rd, (a[0, 0].ctypes.data, c2[0, 0].ctypes.data), 3, 64, 64, capi.p_tree_rule_default())
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x[1:], y[1:]))
    # through the Python mirror, a ragged picture
    W, H = 100, 76
    rule = tr.random_rule(rng)
    got = capi.p_tree_select_rd(a[0, :4], b[0, :4], 2, W, H, rule, with_tree=True)
    exp = rd.tree_select(a[:, :4], b[:, :4], 2, W, H, rule=rule)
    tr.same(got[2], exp[0][0])
    assert np.array_equal(got[0], exp[1][0]) and np.array_equal(got[1], exp[2][0])
