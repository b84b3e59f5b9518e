"""The C-ABI surface of the intra RD estimate with the depth count (no GPU needed: the library loads without one for context-free functions): the three
entry points' declarations with tu_depths before the output pointer, their exports and Python mirror, the header's normative phrases, every entry point
rejected with a NULL context -- and with tu_depths 1 and 4 -- without a byte written, timing slots 36, 37 and 38, and the kernel as further instances of
k_motion_rd.hip."""
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
# entry point -> (arguments, the entry point it mirrors, the argument behind tu_depths)
NEW = {"fhevc_intra_rd_qt_device": (16, "fhevc_intra_rd_device", "fhevc_motion_rd_pu_node* d_out"),
       "fhevc_intra_rd_qt": (10, "fhevc_intra_rd", "fhevc_motion_rd_pu_node* out"),
       "fhevc_p_tree_rd_intra_qt_frame": (18, "fhevc_p_tree_rd_intra_frame", "uint8_t* depth_min")}


def test_declarations_mirror_the_existing_entry_points_with_tu_depths_before_the_output():
    h = _header()
    for sym, (nargs, mirrored, behind) in NEW.items():
        new, old = _args(h, sym), _args(h, mirrored)
        assert len(new) == nargs == len(old) + 1, sym
        at = new.index("int tu_depths")
        assert new[at + 1] == behind and new[:at] + new[at + 1:] == old, sym
        assert new[at - 1] == "int skip_mask", sym
        assert sym in capi.SYMBOLS


def test_exports_and_the_python_mirror():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, (nargs, mirrored, _) in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        new, old = getattr(lib, sym).argtypes, getattr(lib, mirrored).argtypes
        assert len(new) == nargs and len(old) == nargs - 1, sym
        at = [i for i in range(len(old)) if new[i] != old[i]] or [len(old)]
        assert new[at[0]] == C.c_int and list(new[:at[0]]) + list(new[at[0] + 1:]) == list(old), sym
    for name, mirrored in (("intra_rd_qt", "intra_rd"), ("intra_rd_qt_device", "intra_rd_device"), ("p_tree_rd_intra_qt_frame", "p_tree_rd_intra_frame")):
        new, old = list(inspect.signature(getattr(capi.Context, name)).parameters), list(inspect.signature(getattr(capi.Context, mirrored)).parameters)
        assert "tu_depths" in new and [p for p in new if p != "tu_depths"] == old, name
    # further instances of the RD kernel's source, not a source of its own; the first-pass sources are not touched by them
    from fasthevc_amd import build
    assert "k_motion_rd.hip" in build.SOURCES and not any("_qt" in s for s in build.SOURCES) and len(build.SOURCES) == 26
    src = open(os.path.join(build.CSRC, "k_motion_rd.hip")).read()
    assert "fhevc_intra_rd_kernel<int16_t, RdThreeDepths>" in src and "fhevc_intra_rd_kernel<uint8_t, RdThreeDepths>" in src
    assert "fhevc_intra_rd_kernel<int16_t>" in src and "fhevc_intra_rd_kernel<uint8_t>" in src          # the two-depth instances, launched as before
    assert "{ 29, 55, 74, 84 }, { 74, 74, 0, -74 }, { 84, -29, -74, 55 }, { 55, -84, 74, -29 }" in src
    api = open(os.path.join(build.CSRC, "fhevc_motion_api.hip")).read()
    # the entry points without _qt are forwarders with tu_depths 2; the host form goes through the one staging path
    assert api.count("int fhevc_intra_rd_qt(") == 1 and "return fhevc_intra_rd_qt(c, luma, stride_samples, qp, first, fold, rd_merge, skip_mask, 2, out);" in api
    assert re.search(r"return fhevc_intra_rd_qt_device\(c, d_luma, [^;]*skip_mask,\s*2, d_out, stream\);", api)
    assert api.count("upload_pair(") == 2 and "tu_depths == 3 ? 37 : 33" in api


def test_header_phrases():
    h = _header()
    for phrase in ("the intra candidate on HM's full TU tree", "QuadtreeTUMaxDepthIntra 3", "32x32: 32, 16, 8", "16x16: 16, 8, 4", "8x8: 8, 4",
                   "fho_fill_ref(x0, y0, n) ->", "n = 4 included", "z-order availability in 4-sample units", "never selects the\n * smoothed line",
                   "g_as_DST_MAT_4 = { 29, 55, 74, 84 / 74, 74, 0, -74 / 84, -29, -74, 55 / 55, -84, 74, -29 }", "TComRom.cpp:513-517", "TComTrQuant.cpp:412-466",
                   ":876, :898, :945, :969", "keep the DCT", "TEncSearch.cpp:1610-1661", "dSplitCost < dSingleCost ALONE", "K1_i = 256 D1_i + lam (1 + r1_i)",
                   "take1_i = K2_i < K1_i, strictly", "take0 = J1 < J0, strictly", "J1 = 256 sum D1 + lam (1 + sum r1)", "this is not a second definition",
                   "tu_split bits 4..7 mean depth-1 TU i split", "for 8x8 and 64x64 nodes", "there is no new tree kernel", "tu_depths outside {2, 3}",
                   "under slot 37 of fhevc_kernel_timing at tu_depths 3 (36 stays rejected)", "37 = the RD estimate of the intra candidate at three TU depths",
                   "36 is not a slot", "NxN with its four modes"):
        assert phrase in h, phrase
    # the two-depth section still stands beside it
    for phrase in ("An 8x8 node has depth 0 only", "4x4 TUs, and with them the DST, NxN", "fhevc_intra_rd* stays two depths deep", "33 = the RD estimate of the intra candidate",
                   "35 = the RD estimates at three TU depths"):
        assert phrase in h, phrase


def test_rejected_without_a_context_bad_tu_depths_and_the_timing_slots():
    lib = capi.load_library()
    out = np.full(85 * 16 + 1024, CANARY, np.uint8)
    first = np.zeros(85, capi.NODE_DTYPE)
    pic = np.zeros((64, 64), np.int16)
    o, p, f = out.ctypes.data + 512, pic.ctypes.data, first.ctypes.data
    for tud in (2, 3, 1, 4):
        assert lib.fhevc_intra_rd_qt_device(None, p, 2, 64, 4096, 1, 0, 1, 32, f, None, None, 0, tud, o, None) == capi.E_INVALID
        assert lib.fhevc_intra_rd_qt(None, p, 64, 32, f, None, None, 0, tud, o) == capi.E_INVALID
        assert lib.fhevc_p_tree_rd_intra_qt_frame(None, p, p, 64, 32, 4, 0, None, None, 3, tud, o, o + 256, None, None, None, None, None) == capi.E_INVALID
    assert (out == CANARY).all()
    for slot in (36, 37, 38):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID
    # a context needs a GPU: tu_depths 1 and 4 on a live context are the GPU test's; here, that every form checks the argument before it launches or stages
    api = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_motion_api.hip")).read()
    assert api.count("if (!intra_tu_depths_ok(tu_depths)) return fail(c, FHEVC_E_INVALID, kBadTuDepths);") == 2
    assert api.count("if (tu_depths != 2 && tu_depths != 3)") == 4
    timing = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_api.hip")).read()
    assert "if (which != 37)" in timing and "if (which != 35)" in timing and "which > 33" in timing
    ctx = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_ctx.h")).read()
    assert "sum_ms[34]" in ctx and "launches[34]" in ctx and "sum_ms_37" in ctx
