"""The C-ABI surface of the intra RD stage with the NxN candidate of the 8x8 nodes (no GPU needed: the library loads without one for context-free
functions): the three entry points' declarations against the ones they extend, their exports and Python mirror, the record of the plain candidate, the
header's normative phrases with the older sections' sentences still standing, every entry point rejected with a NULL context without a byte written, timing
slots 38, 39 and 40, and the kernel as further instances of k_motion_rd.hip."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from fasthevc_amd import capi
from test_motion_rd_abi import CANARY
from test_motion_rd_qt_abi import _args, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_intra_rd_nxn_device": 17, "fhevc_intra_rd_nxn": 11, "fhevc_p_tree_rd_intra_nxn_frame": 18}


def test_declarations_extend_the_three_depth_entry_points():
    h = _header()
    # the device form: fhevc_intra_rd_qt_device without tu_depths, d_first4 behind d_first, d_nxn behind d_out
    new, old = _args(h, "fhevc_intra_rd_nxn_device"), _args(h, "fhevc_intra_rd_qt_device")
    assert len(new) == 17 and "int tu_depths" not in new
    assert new[new.index("const fhevc_node_cost* d_first") + 1] == "const fhevc_node_cost* d_first4"
    assert new[new.index("fhevc_motion_rd_pu_node* d_out") + 1] == "fhevc_intra_rd_nxn_node* d_nxn" and new[-1] == "void* stream"
    assert [a for a in new if a not in ("const fhevc_node_cost* d_first4", "fhevc_intra_rd_nxn_node* d_nxn")] == [a for a in old if a != "int tu_depths"]
    new, old = _args(h, "fhevc_intra_rd_nxn"), _args(h, "fhevc_intra_rd_qt")
    assert len(new) == 11 and new[new.index("const fhevc_node_cost* first") + 1] == "const fhevc_node_cost* first4" and new[-1] == "fhevc_intra_rd_nxn_node* nxn"
    assert [a for a in new if a not in ("const fhevc_node_cost* first4", "fhevc_intra_rd_nxn_node* nxn")] == [a for a in old if a != "int tu_depths"]
    new, old = _args(h, "fhevc_p_tree_rd_intra_nxn_frame"), _args(h, "fhevc_p_tree_rd_intra_qt_frame")
    assert len(new) == 18 and new[:-1] == [a for a in old if a != "int tu_depths"] and new[-1] == "fhevc_intra_rd_nxn_node* nxn"
    for sym in NEW:
        assert sym in capi.SYMBOLS
    assert re.search(r"#define\s+FHEVC_RD_PART_INTRA_NXN\s+17\b", h) and capi.RD_PART_INTRA_NXN == 17 and capi.RD_PART_INTRA == 16


def test_exports_the_python_mirror_and_the_record():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    assert lib.fhevc_intra_rd_nxn_device.argtypes[4] == C.c_longlong and lib.fhevc_intra_rd_nxn_device.argtypes[13] == C.c_int
    for name in ("intra_rd_nxn", "intra_rd_nxn_device", "p_tree_rd_intra_nxn_frame"):
        assert callable(getattr(capi.Context, name)), name
    assert "first4" in inspect.signature(capi.Context.intra_rd_nxn).parameters and "d_nxn" in inspect.signature(capi.Context.intra_rd_nxn_device).parameters
    assert "with_nxn" in inspect.signature(capi.Context.p_tree_rd_intra_nxn_frame).parameters
    # the record of the plain candidate: 16 bytes without padding, the costs where every RD record keeps them
    dt = capi.INTRA_RD_NXN_DTYPE
    assert dt.itemsize == 16 and [dt.fields[n][1] for n in ("dist", "cost_rd", "bits", "flags", "cbf", "modes")] == [0, 4, 8, 10, 11, 12]
    assert dt.fields["modes"][0].shape == (4,) and dt.fields["cost_rd"][1] == capi.MOTION_RD_PU_DTYPE.fields["cost_rd"][1]
    h = _header()
    m = re.search(r"typedef struct fhevc_intra_rd_nxn_node \{(.*?)\} fhevc_intra_rd_nxn_node;", h, re.S)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+)", m.group(1)) == [("uint32_t", "dist"), ("uint32_t", "cost_rd"), ("uint16_t", "bits"), ("uint8_t", "flags"),
                                                                   ("uint8_t", "cbf"), ("uint8_t", "modes")]
    # further instances of the RD kernel's source behind one more tag, not a source of its own; the existing instances are launched as before
    from fasthevc_amd import build
    assert "k_motion_rd.hip" in build.SOURCES and not any("nxn" in s for s in build.SOURCES) and len(build.SOURCES) == 26
    src = open(os.path.join(build.CSRC, "k_motion_rd.hip")).read()
    for inst in ("fhevc_intra_rd_kernel<int16_t, RdThreeDepths, RdNxN>", "fhevc_intra_rd_kernel<uint8_t, RdThreeDepths, RdNxN>",
                 "fhevc_intra_rd_kernel<int16_t, RdThreeDepths>>", "fhevc_intra_rd_kernel<uint8_t, RdThreeDepths>>", "fhevc_intra_rd_kernel<int16_t>>",
                 "fhevc_intra_rd_kernel<uint8_t>>"):
        assert inst in src, inst
    assert src.index("fhevc_intra_rd_kernel<uint8_t, RdThreeDepths, RdNxN>") > src.rindex("fhevc_motion_rd_kernel<")      # behind every instance there is
    api = open(os.path.join(build.CSRC, "fhevc_motion_api.hip")).read()
    assert api.count("int fhevc_intra_rd_nxn(") == 1 and api.count("upload_pair(") == 2 and "launch_on(c, stream, 39," in api


def test_header_phrases():
    h = _header()
    for phrase in ("the NxN candidate of the 8x8 CUs, four modes", "TEncCu.cpp:806-815", "there is no tu_depths argument", "nodes 21..84",
                   "only satd (dword 0) and the low byte of mode (dword 1) are read", "none of it reaches an address or a loop bound",
                   "(2x, 2y), (2x+1, 2y),\n * (2x, 2y+1), (2x+1, 2y+1): fhevc_intra_p's order", "satd != 0xFFFFFFFF and a mode byte <= 34", "predicts\n * with mode 0 and is dropped",
                   "uiInitTrDepth = 1, TEncSearch.cpp:2187-2188", "fho_fill_ref(x, y, 4) -> fho_pred_intra", "never smoothed",
                   "J = 256 * sum D_i + lam_q8 * (sum r_i + sum bits(m_i))", "cost_rd = min(J >> 8, 0xFFFFFFFE)", "NO split-flag bit is counted", "TEncEntropy.cpp:241-244",
                   "with the 4-point\n * quantiser's numbers", "xCheckBestMode keeps the earlier mode on a tie", "STRICTLY smaller than the 2Nx2N record's or 2Nx2N is invalid",
                   "part = FHEVC_RD_PART_INTRA_NXN (17), tu_split = 1, flags bit 2 set, merged = 0", "64 fhevc_intra_rd_nxn_node per CTU in node order 21..84",
                   "modes 255 four times", "written over exactly its extent", "d_first4 == NULL: every byte and the launch itself are fhevc_intra_rd_qt_device's at 3 (slot 37)",
                   "d_nxn must then be NULL too", "not 4-byte aligned", "Timed under slot 39 of fhevc_kernel_timing (38 stays rejected)", "ONE launch per call",
                   "HM predicts PU i+1 from PU i's reconstruction", "eight candidates plus MPMs per PU", "TEncSearch.cpp:1479",
                   "39 = the RD estimate of the intra candidate with the NxN candidate", "38 is not a slot"):
        assert phrase in h, phrase
    # the older sections still stand, word for word
    for phrase in ("NxN with its four modes", "An 8x8 node has depth 0 only", "4x4 TUs, and with them the DST, NxN", "there is no new tree kernel",
                   "under slot 37 of fhevc_kernel_timing at tu_depths 3 (36 stays rejected)", "37 = the RD estimate of the intra candidate at three TU depths", "36 is not a slot",
                   "fhevc_intra_rd* stays two depths deep"):
        assert phrase in h, phrase
    assert h.index("the NxN candidate of the 8x8 CUs, four modes") > h.index("the intra candidate on HM's full TU tree")


def test_rejected_without_a_context_and_the_timing_slots():
    lib = capi.load_library()
    out = np.full(85 * 16 + 64 * 16 + 2048, CANARY, np.uint8)
    first, first4 = np.zeros(85, capi.NODE_DTYPE), np.zeros(256, capi.NODE_DTYPE)
    pic = np.zeros((64, 64), np.int16)
    o, p, f, f4 = out.ctypes.data + 512, pic.ctypes.data, first.ctypes.data, first4.ctypes.data
    x = o + 85 * 16 + 512
    for a4, ax in ((f4, x), (f4, None), (None, None), (None, x)):
        assert lib.fhevc_intra_rd_nxn_device(None, p, 2, 64, 4096, 1, 0, 1, 32, f, a4, None, None, 0, o, ax, None) == capi.E_INVALID
        assert lib.fhevc_intra_rd_nxn(None, p, 64, 32, f, a4, None, None, 0, o, ax) == capi.E_INVALID
        assert lib.fhevc_p_tree_rd_intra_nxn_frame(None, p, p, 64, 32, 4, 0, None, None, 3, o, o + 256, None, None, None, None, None, ax) == capi.E_INVALID
    assert (out == CANARY).all()
    for slot in (38, 39, 40):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # a context needs a GPU: what a live context does with 38, 39 and 40 is the GPU test's; here, that 39 is a slot beside the table and the others are not
    timing = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_api.hip")).read()
    assert "if (which != 39)" in timing and "which != 38" not in timing and "which != 40" not in timing
    ctx = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_ctx.h")).read()
    assert "sum_ms[34]" in ctx and "sum_ms_39" in ctx and "launches_39" in ctx
