"""The C-ABI surface of the RD stage under a partition size (no GPU needed: the library loads without one for context-free functions): the 16-byte
fhevc_motion_rd_pu_node in the header, in the Python mirror and in the compiled asserts with dword 1, byte 10 and byte 12 where they are read, the
inputs struct, the entry points' signatures and exports, the header's normative phrases, every entry point rejected with a NULL context without a byte
written, timing slots 30, 31 and 32, and the host tree forwarder byte-equal to fhevc_p_tree_select_rd on the same bytes."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import motion_rd_pu_ref as pu
import motion_rd_ref as rd
import p_tree_ref as tr
from fasthevc_amd import capi
from test_motion_rd_abi import CANARY, GEOMETRIES, host_tree, random_rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_motion_rd_pu_device": 14, "fhevc_motion_rd_pu": 9, "fhevc_p_tree_select_rd_pu": 9, "fhevc_p_tree_select_rd_pu_device": 12, "fhevc_p_tree_rd_frame": 16}


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def _struct(h, name):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", h)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]


def test_struct_size_and_offsets():
    d = capi.MOTION_RD_PU_DTYPE
    assert d.itemsize == 16 and d.names == ("dist", "cost_rd", "bits", "flags", "tu_split", "part", "merged", "pad")
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 10, 11, 12, 13, 14]
    # bytes 0..11 are the RD record's; dword 1 and byte 10 are where the tree kernels read; byte 12 / 13 of a selection record are best / second
    r = capi.MOTION_RD_DTYPE
    assert all(d.fields[n][:2] == r.fields[n][:2] for n in ("dist", "cost_rd", "bits", "flags", "tu_split"))
    assert d.fields["cost_rd"][1] == capi.SHAPE_DTYPE.fields["cost_best"][1] == 4 and d.fields["flags"][1] == capi.MOTION_SKIP_DTYPE.fields["flags"][1] == 10
    assert capi.SHAPE_DTYPE.fields["best"][1] == 12 and capi.SHAPE_DTYPE.fields["second"][1] == 13 and d.fields["part"][1] == 12
    assert (capi.RD_PART_BEST, capi.RD_PART_SECOND) == (8, 9) and pu.INVALID == (rd.MARK, rd.MARK, 0xFFFF, 0, 0, 255, 0, (0, 0))
    h = _header()
    assert _struct(h, "fhevc_motion_rd_pu_node") == ["uint32_t dist", "uint32_t cost_rd", "uint16_t bits", "uint8_t flags", "uint8_t tu_split", "uint8_t part",
                                                     "uint8_t merged", "uint8_t pad[2]"]
    assert _struct(h, "fhevc_motion_rd_pu_inputs") == ["const fhevc_motion_qpel_node *nodes, *pus, *pus_small", "const fhevc_motion_merge_node *merge_pus, *merge_pus_small",
                                                       "const fhevc_motion_mvp *mvp_nodes, *mvp_pus, *mvp_pus_small", "const fhevc_pu_shape_node *shapes",
                                                       "const fhevc_motion_rd_pu_node *fold"]
    assert C.sizeof(capi.MotionRdPuInputs) == 80 and [f[0] for f in capi.MotionRdPuInputs._fields_] == [
        "nodes", "pus", "pus_small", "merge_pus", "merge_pus_small", "mvp_nodes", "mvp_pus", "mvp_pus_small", "shapes", "fold"]
    # ... pinned where they are compiled, too
    internal = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_internal.h")).read()
    assert "sizeof(FhevcMotionRdPuNode) == 16 && offsetof(FhevcMotionRdPuNode, cost_rd) == 4 && offsetof(FhevcMotionRdPuNode, flags) == 10" in internal
    assert "offsetof(FhevcMotionRdPuNode, part) == 12" in internal
    api = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_motion_api.hip")).read()
    assert "sizeof(fhevc_motion_rd_pu_node) == 16 && offsetof(fhevc_motion_rd_pu_node, cost_rd) == 4 && offsetof(fhevc_motion_rd_pu_node, flags) == 10" in api
    assert "offsetof(fhevc_motion_rd_pu_node, part) == 12" in api and "offsetof(fhevc_pu_shape_node, best) == 12" in api


def test_header_python_mirror_and_exports():
    h = _header()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym, nargs in NEW.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m and len(strip(m.group(1)).split(",")) == nargs, sym
        assert sym in capi.SYMBOLS
    assert "fhevc_ctx" not in re.search(r"\bint\s+fhevc_p_tree_select_rd_pu\s*\(([^;]*)\);", h).group(1)
    for phrase in ("31 = the RD estimate under a partition size", "30 is not a slot", "Timed under slot 31", "TComDataCU.cpp:1478-1503", "QuadtreeTUMaxDepthInter == 1",
                   "uiMRGCost < uiMECost", "getPartIndexAndSize", "xCheckBestMode keeps the earlier mode", "fold == d_out is allowed", "AMP at level 3",
                   "A marker loses to anything", "part mode and of the merge flags are left out", "part_mode outside {0, 1, 2, 4..9}", "side_bits is the sum over the parts",
                   "word for word those of", "two of the seven partition sizes", "28 is not a slot", "29 = the RD estimate"):
        assert phrase in h, phrase
    sig = inspect.signature(capi.Context.motion_rd_pu)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "part_mode", "nodes", "pus", "pus_small", "merge_pus", "merge_pus_small", "mvp_nodes", "mvp_pus",
                                    "mvp_pus_small", "shapes", "fold", "origin", "stride", "qp", "max_range"]
    sig = inspect.signature(capi.Context.motion_rd_pu_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "part_mode", "inputs", "d_out", "rows", "stream", "qp",
                                    "max_range"]
    sig = inspect.signature(capi.Context.p_tree_select_rd_pu_device)
    assert list(sig.parameters) == ["self", "d_rd_pu", "d_rd_merge", "skip_mask", "num_pictures", "d_depth_min", "d_depth_max", "d_tree", "rows", "stream", "rule"]
    assert hasattr(capi, "p_tree_select_rd_pu") and hasattr(capi.Context, "p_tree_rd_frame")
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    # the stage is a further instantiation of the RD kernel's source, not a source of its own
    from fasthevc_amd import build
    assert "k_motion_rd.hip" in build.SOURCES and not any("rd_pu" in s for s in build.SOURCES)
    src = open(os.path.join(build.CSRC, "k_motion_rd.hip")).read()
    assert "template <typename T, int MR, bool PU, class... A>" in src and "if constexpr (PU)" in src


def test_rejected_without_a_context_and_the_timing_slots():
    lib = capi.load_library()
    out = np.full(85 * 16 + 512, CANARY, np.uint8)
    rec = np.zeros(85, capi.MOTION_QPEL_DTYPE)
    pic = np.zeros((64, 64), np.int16)
    inputs = capi.MotionRdPuInputs(nodes=rec.ctypes.data)
    o = out.ctypes.data
    assert lib.fhevc_motion_rd_pu_device(None, pic.ctypes.data, 2, 64, 4096, 2, 0, 1, 32, 4, 0, C.byref(inputs), o, None) == capi.E_INVALID
    assert lib.fhevc_motion_rd_pu(None, pic.ctypes.data, pic.ctypes.data, 64, 32, 4, 0, C.byref(inputs), o) == capi.E_INVALID
    assert lib.fhevc_p_tree_select_rd_pu_device(None, rec.ctypes.data, rec.ctypes.data, 1, 1, 0, 1, None, o, None, None, None) == capi.E_INVALID
    assert lib.fhevc_p_tree_rd_frame(None, pic.ctypes.data, pic.ctypes.data, 64, 32, 4, 0, None, None, 3, o, o + 256, None, None, None, None) == capi.E_INVALID
    assert (out == CANARY).all()
    for slot in (30, 31, 32):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # the host form of the tree: what fhevc_p_tree_select_rd rejects
    rng = np.random.default_rng(5)
    a, b = random_pu(rng, (85,)), random_rd(rng, (85,))
    d = capi.p_tree_rule_default()
    call = lambda **kw: host_tree(lib.fhevc_p_tree_select_rd_pu, (kw.get("a", a.ctypes.data), kw.get("b", b.ctypes.data)), kw.get("mask", 3), kw.get("vw", 64),
                                  kw.get("vh", 64), kw.get("rule", d), kw.get("want", (True, True, True)))
    assert call()[0] == capi.OK
    for change in (dict(a=None), dict(b=None), dict(mask=-1), dict(mask=4), dict(rule=None), dict(vw=7), dict(vh=65), dict(want=(False, False, False))):
        assert call(**change)[0] == capi.E_INVALID, change            # host_tree asserts that nothing was written


def random_pu(rng, shape):
    """folded records of random bytes, one in seven a marker's cost"""
    a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 16), capi.MOTION_RD_PU_DTYPE).reshape(shape).copy()
    a["cost_rd"] = np.where(rng.random(shape) < 1 / 7, rd.MARK, a["cost_rd"] % 100000)
    return a


def test_the_forwarder_is_the_rd_tree_on_the_same_bytes():
    """48 CTUs x 4 masks: every output byte of fhevc_p_tree_select_rd_pu equals fhevc_p_tree_select_rd's on the records reinterpreted, and the restatement"""
    lib = capi.load_library()
    rng = np.random.default_rng(412)
    n = 48
    a, b = random_pu(rng, (1, n, 85)), random_rd(rng, (1, n, 85))
    for c in range(n):
        vw, vh = GEOMETRIES[c % len(GEOMETRIES)]
        rule = tr.random_rule(rng) if c % 3 else capi.p_tree_rule_default()
        for mask in range(4):
            got = host_tree(lib.fhevc_p_tree_select_rd_pu, (a[0, c].ctypes.data, b[0, c].ctypes.data), mask, vw, vh, rule)
            base = host_tree(lib.fhevc_p_tree_select_rd, (a[0, c].ctypes.data, b[0, c].ctypes.data), mask, vw, vh, rule)
            assert got[0] == base[0] == capi.OK and all(x.tobytes() == y.tobytes() for x, y in zip(got[1:], base[1:])), (c, mask)
            erec, emin, emax = (x[0, 0] for x in rd.tree_select(a[:, c:c + 1], b[:, c:c + 1], mask, vw, vh, rule=rule))
            tr.same(got[3].view(capi.TREE_DTYPE), erec, (c, mask))
            assert np.array_equal(got[1], emin) and np.array_equal(got[2], emax)
    # part, merged and pad are no input of the tree
    c2 = a.copy()
    c2["part"] ^= 0xFF
    c2["merged"] ^= 3
    x = host_tree(lib.fhevc_p_tree_select_rd_pu, (a[0, 0].ctypes.data, b[0, 0].ctypes.data), 3, 64, 64, capi.p_tree_rule_default())
    y = host_tree(lib.fhevc_p_tree_select_rd_pu, (c2[0, 0].ctypes.data, b[0, 0].ctypes.data), 3, 64, 64, capi.p_tree_rule_default())
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x[1:], y[1:]))
    # through the Python mirror, a ragged picture
    W, H = 100, 76
    rule = tr.random_rule(rng)
    got = capi.p_tree_select_rd_pu(a[0, :4], b[0, :4], 2, W, H, rule, with_tree=True)
    exp = capi.p_tree_select_rd(a[0, :4].view(capi.MOTION_RD_DTYPE), b[0, :4], 2, W, H, rule, with_tree=True)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(got, exp))
