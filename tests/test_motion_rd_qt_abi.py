"""The C-ABI surface of the RD stages with the depth count (no GPU needed: the library loads without one for context-free functions): the five entry
points' declarations with tu_depths before the output pointer, their exports and Python mirror, the header's normative phrases, every entry point rejected
with a NULL context -- and with tu_depths 1 and 4 -- without a byte written, timing slots 34, 35 and 36, and the kernel as further instances of
k_motion_rd.hip."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from fasthevc_amd import capi
from test_motion_rd_abi import CANARY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry point -> (arguments, the entry point it mirrors, the argument behind tu_depths)
NEW = {"fhevc_motion_rd_qt_device": (16, "fhevc_motion_rd_device", "fhevc_motion_rd_node* d_out"),
       "fhevc_motion_rd_qt": (11, "fhevc_motion_rd", "fhevc_motion_rd_node* out"),
       "fhevc_motion_rd_pu_qt_device": (15, "fhevc_motion_rd_pu_device", "fhevc_motion_rd_pu_node* d_out"),
       "fhevc_motion_rd_pu_qt": (10, "fhevc_motion_rd_pu", "fhevc_motion_rd_pu_node* out"),
       "fhevc_p_tree_rd_qt_frame": (17, "fhevc_p_tree_rd_frame", "uint8_t* depth_min")}


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def _args(h, sym):
    m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
    assert m, sym
    return [re.sub(r"\s+", " ", a).strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_declarations_mirror_the_existing_entry_points_with_tu_depths_before_the_output():
    h = _header()
    for sym, (nargs, mirrored, behind) in NEW.items():
        new, old = _args(h, sym), _args(h, mirrored)
        assert len(new) == nargs == len(old) + 1, sym
        at = new.index("int tu_depths")
        assert new[at + 1] == behind and new[:at] + new[at + 1:] == old, sym
        assert sym in capi.SYMBOLS


def test_exports_and_the_python_mirror():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, (nargs, mirrored, _) in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        new, old = getattr(lib, sym).argtypes, getattr(lib, mirrored).argtypes
        assert len(new) == nargs and C.c_int in new and len(old) == nargs - 1, sym
    for name, mirrored in (("motion_rd_qt", "motion_rd"), ("motion_rd_qt_device", "motion_rd_device"), ("motion_rd_pu_qt", "motion_rd_pu"),
                           ("motion_rd_pu_qt_device", "motion_rd_pu_device"), ("p_tree_rd_qt_frame", "p_tree_rd_frame")):
        new, old = list(inspect.signature(getattr(capi.Context, name)).parameters), list(inspect.signature(getattr(capi.Context, mirrored)).parameters)
        assert "tu_depths" in new and [p for p in new if p != "tu_depths"] == old, name
    # further instances of the RD kernel's source, not a source of its own
    from fasthevc_amd import build
    assert "k_motion_rd.hip" in build.SOURCES and not any("_qt" in s for s in build.SOURCES)
    src = open(os.path.join(build.CSRC, "k_motion_rd.hip")).read()
    assert "struct RdThreeDepths" in src and "rd_depth<2, T, QT>" in src and "kFineTus = 16 + 64" in src
    api = open(os.path.join(build.CSRC, "fhevc_motion_api.hip")).read()
    # the host forms go through the one staging path: no second upload of the pair, no second copy of the existing forms' bodies
    assert api.count("int fhevc_motion_rd_qt(") == 1 and "return fhevc_motion_rd_qt(c, cur_luma, ref_luma, stride_samples, qp, max_range, source, in, mvp, 2, out);" in api
    assert "return fhevc_motion_rd_pu_qt(c, cur_luma, ref_luma, stride_samples, qp, max_range, part_mode, inputs, 2, out);" in api
    assert api.count("upload_pair(") == 2


def test_header_phrases():
    h = _header()
    for phrase in ("the third TU depth (further instances of k_motion_rd.hip)", "32 -> 32, 16, 8 and 16 -> 16, 8, 4", "TEncSearch.cpp:5020-5134", "TEncSearch.cpp:4556-5160",
                   "K1_i = 256 D1_i + lam (1 + r1_i)", "K2_i = 256 sum D2 + lam (1 + sum r2)", "take1_i = (some child has a non-zero level) AND K2_i < K1_i, strictly",
                   "coded_i = take1_i OR cbf1_i", ":5093-5101", "J1 = sum C_i + lam", "take0 = (some coded_i) AND J1 < J0", "four flag bits MORE",
                   "tu_split gains bits 4..7", "these bits are zero unless bit 0 is set", "Bits 1..3 stay the 64x64 node's", "there is no new tree kernel",
                   "tu_depths outside {2, 3}", "Timed under slot 35", "34 stays rejected", "35 = the RD estimates at three TU depths", "34 is not a slot",
                   "special case of this definition", "fhevc_intra_rd* stays two depths deep", "the two sides of every comparison"):
        assert phrase in h, phrase
    # the text of the two-depth sections still stands beside it
    for phrase in ("29 = the RD estimate", "31 = the RD estimate under a partition size", "33 = the RD estimate of the intra candidate", "32 is not a slot"):
        assert phrase in h, phrase


def test_rejected_without_a_context_bad_tu_depths_and_the_timing_slots():
    lib = capi.load_library()
    out = np.full(85 * 16 + 1024, CANARY, np.uint8)
    rec = np.zeros(85, capi.MOTION_QPEL_DTYPE)
    pic = np.zeros((64, 64), np.int16)
    inputs = capi.MotionRdPuInputs(nodes=rec.ctypes.data)
    o, p, r = out.ctypes.data, pic.ctypes.data, rec.ctypes.data
    for tud in (2, 3, 1, 4):
        assert lib.fhevc_motion_rd_qt_device(None, p, 2, 64, 4096, 2, 0, 1, 32, 4, 1, r, None, tud, o, None) == capi.E_INVALID
        assert lib.fhevc_motion_rd_qt(None, p, p, 64, 32, 4, 1, r, None, tud, o) == capi.E_INVALID
        assert lib.fhevc_motion_rd_pu_qt_device(None, p, 2, 64, 4096, 2, 0, 1, 32, 4, 0, C.byref(inputs), tud, o, None) == capi.E_INVALID
        assert lib.fhevc_motion_rd_pu_qt(None, p, p, 64, 32, 4, 0, C.byref(inputs), tud, o) == capi.E_INVALID
        assert lib.fhevc_p_tree_rd_qt_frame(None, p, p, 64, 32, 4, 0, None, None, 3, tud, o, o + 256, None, None, None, None) == capi.E_INVALID
    assert (out == CANARY).all()
    for slot in (34, 35, 36):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # a context needs a GPU: tu_depths 1 and 4 on a live context are the GPU test's; here, that every form checks the argument before it launches or stages
    api = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_motion_api.hip")).read()
    assert api.count("if (tu_depths != 2 && tu_depths != 3)") == 4 and "with_rd->tu_depths != 2 && with_rd->tu_depths != 3" in api
    assert "if (which != 35)" in open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_api.hip")).read()
