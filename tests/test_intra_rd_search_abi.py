"""The C-ABI surface of the intra RD stage that searches the first pass's candidate lists (no GPU needed: the library loads without one for context-free
functions): the entry points' declarations against the ones they extend, their exports and Python mirror, the 8-byte rule and its default, the header's
normative phrases with the older sections' sentences still standing, every entry point rejected with a NULL context without a byte written, timing slots
40, 41 and 42, and the kernel as further instances of k_motion_rd.hip."""
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
NEW = {"fhevc_intra_rd_search_device": 20, "fhevc_intra_rd_search": 14, "fhevc_p_tree_rd_intra_search_frame": 19, "fhevc_intra_search_rule_default": 1}
LISTS = ["const uint8_t* d_modes", "int list_stride", "const uint8_t* d_modes4", "int list_stride4", "const fhevc_intra_search_rule* rule"]


def test_declarations_extend_the_nxn_entry_points():
    h = _header()
    # the device form: fhevc_intra_rd_nxn_device with the two lists, their strides and the rule in the two record arrays' place
    new, old = _args(h, "fhevc_intra_rd_search_device"), _args(h, "fhevc_intra_rd_nxn_device")
    assert len(new) == 20 and new[9:14] == LISTS and new[-1] == "void* stream"
    assert new[:9] + new[14:] == [a for a in old if a not in ("const fhevc_node_cost* d_first", "const fhevc_node_cost* d_first4")]
    new, old = _args(h, "fhevc_intra_rd_search"), _args(h, "fhevc_intra_rd_nxn")
    assert len(new) == 14 and new[4:9] == [a.replace("d_modes", "modes") for a in LISTS] and new[-1] == "fhevc_intra_rd_nxn_node* nxn"
    assert new[:4] + new[9:] == [a for a in old if a not in ("const fhevc_node_cost* first", "const fhevc_node_cost* first4")]
    new, old = _args(h, "fhevc_p_tree_rd_intra_search_frame"), _args(h, "fhevc_p_tree_rd_intra_nxn_frame")
    assert len(new) == 19 and [a for a in new if a != "const fhevc_intra_search_rule* rule"] == old
    assert new[new.index("const fhevc_p_tree_rule* tree_rule") + 1] == "const fhevc_intra_search_rule* rule"
    for sym in NEW:
        assert sym in capi.SYMBOLS


def test_exports_the_python_mirror_the_rule_and_its_default():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym
    assert lib.fhevc_intra_rd_search_device.argtypes[4] == C.c_longlong and lib.fhevc_intra_rd_search_device.argtypes[10] == C.c_int
    for name in ("intra_rd_search", "intra_rd_search_device", "p_tree_rd_intra_search_frame"):
        assert callable(getattr(capi.Context, name)), name
    assert "modes4" in inspect.signature(capi.Context.intra_rd_search).parameters and "rule" in inspect.signature(capi.Context.intra_rd_search_device).parameters
    # the rule: 8 bytes without padding, as a ctypes structure and as a record
    assert C.sizeof(capi.IntraSearchRule) == 8 and capi.INTRA_SEARCH_RULE_DTYPE.itemsize == 8
    dt = capi.INTRA_SEARCH_RULE_DTYPE
    assert [dt.fields[n][1] for n in ("count", "count4", "append_planar", "pad")] == [0, 4, 5, 6]
    assert [getattr(capi.IntraSearchRule, n).offset for n in ("count", "count4", "append_planar", "pad")] == [0, 4, 5, 6]
    h = _header()
    m = re.search(r"typedef struct fhevc_intra_search_rule \{(.*?)\} fhevc_intra_search_rule;", h, re.S)
    assert m and re.findall(r"(uint\d+_t)\s+(\w+)", m.group(1)) == [("uint8_t", "count"), ("uint8_t", "count4"), ("uint8_t", "append_planar"), ("uint8_t", "pad")]
    # HM's numbers; every byte is written, and a null rule is left alone
    raw = (C.c_uint8 * 8)(*([CANARY] * 8))
    lib.fhevc_intra_search_rule_default(C.cast(raw, C.POINTER(capi.IntraSearchRule)))
    assert list(raw) == [3, 3, 3, 8, 8, 1, 0, 0]
    lib.fhevc_intra_search_rule_default(None)
    r = capi.intra_search_rule_default()
    assert list(r.count) == [3, 3, 3, 8] and r.count4 == 8 and r.append_planar == 1 and list(r.pad) == [0, 0]
    # further instances of the RD kernel's source behind one more tag, not a source of its own; the existing instances are launched as before
    from fasthevc_amd import build
    assert "k_motion_rd.hip" in build.SOURCES and not any("search" in s for s in build.SOURCES) and len(build.SOURCES) == 26
    src = open(os.path.join(build.CSRC, "k_motion_rd.hip")).read()
    for inst in ("fhevc_intra_rd_kernel<int16_t, RdThreeDepths, RdSearch>", "fhevc_intra_rd_kernel<uint8_t, RdThreeDepths, RdSearch>",
                 "fhevc_intra_rd_kernel<int16_t, RdThreeDepths, RdNxN>", "fhevc_intra_rd_kernel<uint8_t, RdThreeDepths, RdNxN>"):
        assert inst in src, inst
    assert src.index("fhevc_intra_rd_kernel<int16_t, RdThreeDepths, RdSearch>") > src.rindex("RdThreeDepths, RdNxN>")      # behind every instance there is
    api = open(os.path.join(build.CSRC, "fhevc_motion_api.hip")).read()
    assert api.count("int fhevc_intra_rd_search(") == 1 and api.count("upload_pair(") == 2 and "launch_on(c, stream, 41," in api


def test_header_phrases():
    h = _header()
    for phrase in ("the intra candidate searched over the first pass's candidate lists", "TEncSearch.cpp:2244, g_aucIntraModeNumFast_UseMPM", ":2297-2320", ":2349-2480",
                   "85 * list_stride bytes per CTU, best\n * first, compact over the band", "256 * list_stride4 bytes per CTU", "No byte reaches an address or a loop bound",
                   "Bytes > 34 are\n * skipped", "iff the list has at least one valid entry and none of them is 0", "TComDataCU.cpp:1403-1421",
                   "MPMs from coded intra neighbours stay a stated departure", "A node is valid iff it is INSIDE and its list is not empty", "Step A (bCheckFirst)",
                   "A_c = sum over the node's depth-0 TUs of J0 (the fhevc_intra_rd_qt J0, predicted at m_c) + lam * bits(m_c), in 64 bits",
                   "a candidate strictly below the best becomes the best, and the old best becomes the second", "candidate strictly below the second becomes the second",
                   "iff a second exists and its cost_rd is STRICTLY smaller, compared on the unshifted 64-bit J", "pad[1] = the winner's position in the list",
                   "the appended planar counts as the position behind the last list byte\n * used", "256 D + lam (r + bits(m)) wins, strict < in list order",
                   "With\n * d_modes4 NULL there is no NxN candidate, and d_nxn must be NULL", "a null d_modes or rule; strides outside 1..8; a count of 0,\n * or a count above its stride",
                   "append_planar above 1, or a non-zero pad; d_nxn without d_modes4; any overlap of an input list with an output",
                   "Timed under slot 41 of fhevc_kernel_timing (40 and 42 stay rejected)", "F(m).J <= A(m)", "ONE launch per call", "HM: count {3, 3, 3, 8}, count4 8, append_planar 1",
                   "41 = the RD estimate of the intra candidate searched over the first pass's candidate lists", "40 is not a slot"):
        assert phrase in h, phrase
    # the older sections still stand, word for word
    for phrase in ("HM's RD search over the candidate list", "eight candidates plus MPMs per PU -- here there is one mode per PU", "Timed under slot 39 of fhevc_kernel_timing (38 stays rejected)",
                   "39 = the RD estimate of the intra candidate with the NxN candidate", "38 is not a slot", "d_first4 == NULL: every byte and the launch itself are fhevc_intra_rd_qt_device's at 3 (slot 37)"):
        assert phrase in h, phrase
    assert h.index("the intra candidate searched over the first pass's candidate lists") > h.index("the NxN candidate of the 8x8 CUs, four modes")


def test_rejected_without_a_context_and_the_timing_slots():
    lib = capi.load_library()
    out = np.full(85 * 16 + 64 * 16 + 2048, CANARY, np.uint8)
    modes, modes4 = np.zeros(85 * 8, np.uint8), np.zeros(256 * 8, np.uint8)
    pic = np.zeros((64, 64), np.int16)
    rule = capi.intra_search_rule_default()
    o, p, m, m4 = out.ctypes.data + 512, pic.ctypes.data, modes.ctypes.data, modes4.ctypes.data
    x = o + 85 * 16 + 512
    for a4, ax in ((m4, x), (m4, None), (None, None), (None, x)):
        assert lib.fhevc_intra_rd_search_device(None, p, 2, 64, 4096, 1, 0, 1, 32, m, 8, a4, 8, C.byref(rule), None, None, 0, o, ax, None) == capi.E_INVALID
        assert lib.fhevc_intra_rd_search(None, p, 64, 32, m, 8, a4, 8, C.byref(rule), None, None, 0, o, ax) == capi.E_INVALID
        assert lib.fhevc_p_tree_rd_intra_search_frame(None, p, p, 64, 32, 4, 0, None, None, C.byref(rule), 3, o, o + 256, None, None, None, None, None, ax) == capi.E_INVALID
    assert (out == CANARY).all()
    for slot in (40, 41, 42):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # a context needs a GPU: what a live context does with 40, 41 and 42 is the GPU test's; here, that 41 is a slot beside the table and the others are not
    timing = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_api.hip")).read()
    assert "if (which != 41)" in timing and "which != 40" not in timing and "which != 42" not in timing
    ctx = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_ctx.h")).read()
    assert "sum_ms[34]" in ctx and "sum_ms_41" in ctx and "launches_41" in ctx and "sum_ms_39" in ctx
