"""The C-ABI surface of the RD estimate of the intra candidate (no GPU needed: the library loads without one for context-free functions): the entry
points' declarations and exports, FHEVC_RD_PART_INTRA in header, mirror and compiled asserts, the record offsets the stage relies on (dword 1, byte 10,
byte 12, the mode in byte 14; satd and mode of the first-pass record), the header's normative phrases, every entry point rejected with a NULL context
without a byte written, and timing slots 32, 33 and 34."""
import inspect
import os
import re
import subprocess

import numpy as np

import intra_rd_ref as ir
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_intra_rd_device": 15, "fhevc_intra_rd": 9, "fhevc_p_tree_rd_intra_frame": 17}
CANARY = 0xA5


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def test_the_constant_and_the_record_offsets():
    h = _header()
    assert re.search(r"#define\s+FHEVC_RD_PART_INTRA\s+16\b", h) and capi.RD_PART_INTRA == ir.PART_INTRA == 16
    assert capi.RD_PART_INTRA not in (0, 1, 2, 3, 4, 5, 6, 7, capi.RD_PART_BEST, capi.RD_PART_SECOND, 255)
    d = capi.MOTION_RD_PU_DTYPE
    assert d.itemsize == 16 and [d.fields[n][1] for n in ("cost_rd", "flags", "tu_split", "part", "merged", "pad")] == [4, 10, 11, 12, 13, 14]
    n = capi.NODE_DTYPE
    assert n.itemsize == 16 and n.fields["satd"][1] == 0 and n.fields["mode"][1] == 4
    assert tuple(ir.MARKER.tolist()[:7]) == (ir.MARK, ir.MARK, 0xFFFF, 0, 0, 255, 0)
    # ... pinned where they are compiled, too
    internal = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_internal.h")).read()
    assert "constexpr int kRdPartIntra = 16;" in internal and "fhevc_launch_intra_rd(" in internal
    api = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_motion_api.hip")).read()
    assert "FHEVC_RD_PART_INTRA == kRdPartIntra" in api and "offsetof(fhevc_motion_rd_pu_node, pad) == 14" in api
    assert "offsetof(fhevc_node_cost, satd) == 0 && offsetof(fhevc_node_cost, mode) == 4" in api
    kernel = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "k_motion_rd.hip")).read()
    assert "offsetof(FhevcNodeCost, satd) == 0 && offsetof(FhevcNodeCost, mode) == 4" in kernel and "fhevc_intra_rd_kernel" in kernel


def test_header_python_mirror_and_exports():
    h = _header()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym, nargs in NEW.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m and len(strip(m.group(1)).split(",")) == nargs, sym
        assert sym in capi.SYMBOLS
    for phrase in ("33 = the RD estimate of the intra candidate", "32 is not a slot", "Timed under slot 33", "TEncSearch.cpp:1661 against :5117", "dSplitCost < dSingleCost alone",
                   "TEncCu.cpp:799-804", "There is no frame pairing", "only satd (dword 0) and the low byte of mode (dword 1) are read", "an invalid node predicts with mode 0",
                   "fho_fill_ref, fho_filter_ref, fho_use_filtered_ref, fho_pred_intra", "An 8x8 node has depth 0 only", "d_fold == d_out is allowed",
                   "keeps the earlier mode on a tie", "part = FHEVC_RD_PART_INTRA", "pad[0] = the mode", "4x4 TUs, and with them the DST, NxN", "the mode-flag bits",
                   "the margin fit and any hook", "reconstructed neighbours", "There is no new tree kernel", "A\n * rejected call moves nothing",
                   # the sentences of the earlier stages stand as they were
                   "31 = the RD estimate under a partition size", "30 is not a slot", "29 = the RD estimate", "fold == d_out is allowed"):
        assert phrase in h, phrase
    assert list(inspect.signature(capi.Context.intra_rd).parameters) == ["self", "plane", "first", "fold", "rd_merge", "skip_mask", "origin", "stride", "qp"]
    assert list(inspect.signature(capi.Context.intra_rd_device).parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_first", "d_out",
                                                                                "d_fold", "d_rd_merge", "skip_mask", "rows", "stream", "qp"]
    assert list(inspect.signature(capi.Context.p_tree_rd_intra_frame).parameters)[-5:] == ["with_shapes", "with_merge", "with_rd_merge", "with_rd_pu", "with_first"]
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    # the stage lives beside the transform code it shares, not in a source of its own
    from fasthevc_amd import build
    assert "k_motion_rd.hip" in build.SOURCES and not any("intra_rd" in s for s in build.SOURCES)


def test_rejected_without_a_context_and_the_timing_slots():
    lib = capi.load_library()
    out = np.full(85 * 16 + 1024, CANARY, np.uint8)
    first = np.zeros(85, capi.NODE_DTYPE)
    rec = np.zeros(85, capi.MOTION_RD_PU_DTYPE)
    pic = np.zeros((64, 64), np.int16)
    o = out.ctypes.data + 256
    assert lib.fhevc_intra_rd_device(None, pic.ctypes.data, 2, 64, 4096, 1, 0, 1, 32, first.ctypes.data, rec.ctypes.data, rec.ctypes.data, 3, o, None) == capi.E_INVALID
    assert lib.fhevc_intra_rd(None, pic.ctypes.data, 64, 32, first.ctypes.data, rec.ctypes.data, rec.ctypes.data, 3, o) == capi.E_INVALID
    assert lib.fhevc_p_tree_rd_intra_frame(None, pic.ctypes.data, pic.ctypes.data, 64, 32, 4, 0, None, None, 3, o, o + 256, None, None, None, None, o + 512) == capi.E_INVALID
    assert (out == CANARY).all()
    for slot in (32, 33, 34):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # which numbers are slots is decided before a context is needed for anything else: the source says 33 is one, 32 and 34 are none
    api = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_api.hip")).read()
    m = re.search(r"if \(!c \|\| which < 0 \|\| which > (\d+) \|\| ([^)]*)\) return FHEVC_E_INVALID;", api)
    assert m and int(m.group(1)) == 33 and "which == 32" in m.group(2) and "which == 33" not in m.group(2)
    ctx_h = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_ctx.h")).read()
    assert "double sum_ms[34]" in ctx_h and "uint64_t launches[34]" in ctx_h
