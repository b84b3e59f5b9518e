"""The C-ABI surface of the quarter-sample refinements at HM's SearchRange (no GPU needed): include/fasthevc.h declares fhevc_motion_refine_pu_wide
and fhevc_motion_refine_pu_wide_device, states the contract (max_range 1..64, the pair rules, no state between calls) and documents timing slot 12
behind slots 0..11 as they read; the comments that spoke of the gap point to the new entry point; fasthevc_amd/capi.py mirrors it; the built library
exports it; each entry point refuses a NULL context before it touches a device."""
import inspect
import os
import re
import subprocess

from fasthevc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fhevc_motion_refine_pu_wide_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                           "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int max_range",
                                           "const fhevc_motion_node* d_nodes", "fhevc_motion_qpel_node* d_out_nodes",
                                           "const fhevc_motion_node* d_pus", "fhevc_motion_qpel_node* d_out_pus",
                                           "const fhevc_motion_node* d_pus_small", "fhevc_motion_qpel_node* d_out_pus_small", "void* stream"],
    "fhevc_motion_refine_pu_wide": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int max_range",
                                    "const fhevc_motion_node* nodes", "fhevc_motion_qpel_node* out_nodes",
                                    "const fhevc_motion_node* pus", "fhevc_motion_qpel_node* out_pus",
                                    "const fhevc_motion_node* pus_small", "fhevc_motion_qpel_node* out_pus_small"],
}


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def test_header_declares_the_entry_points_and_states_the_contract():
    h = _header()
    for sym, args in ARGS.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m, sym
        got = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert len(got) == len(args), (sym, got)
        for g, a in zip(got, args):
            assert g == a or (a == "fhevc_ctx*" and re.fullmatch(r"fhevc_ctx\s*\*\s*\w*", g)), (sym, g, a)
    for words in (r"max_range 1\.\.64", r"max_range outside 1\.\.64", r"Each in / out pair may be NULL together", r"neither computed nor written",
                  r"All three pairs NULL, or a pair with exactly\s+\*?\s*one NULL member, is FHEVC_E_INVALID", r"ALWAYS\s+\*?\s*SATD, whatever fhevc_set_motion_distortion says",
                  r"s_acMvRefineH, then the quarter-sample stage of s_acMvRefineQ", r"byte for byte\s+\*?\s*what that entry point writes",
                  r"byte for byte what fhevc_motion_refine_pu_device writes", r"keeps NO state in HBM between calls",
                  r"Timed under slot 12 of fhevc_kernel_timing, each launch counted"):
        assert re.search(words, h), words
    # the comments that spoke of the gap keep their words and point to the new entry point
    assert re.search(r"Not covered: the quarter-sample refinement\s+\*?\s*of PU vectors beyond \+-8 \(fhevc_motion_refine_pu marks them\)", h)
    assert re.search(r"fhevc_motion_refine_pu_wide, below, refines the vectors of all three outputs at max_range 1\.\.64", h)
    assert re.search(r"\(1\.\.8: no PU search writes longer vectors, so the 15\.5 KB window serves\)", h)
    assert re.search(r"ranges above 8 \(fhevc_motion_search_pu_wide\) are fhevc_motion_refine_pu_wide's, below", h)
    assert re.search(r"max_range outside 1\.\.8", h)        # fhevc_motion_refine_pu_device keeps its own guard


def test_timing_slots_0_to_11_read_as_before_and_slot_12_is_appended():
    h = re.sub(r"\s*\n \*\s*", " ", _header())
    assert ("which: 0 = depth CNN, 1 = source Hadamard, 2 = first pass, 3 = pre-analysis, 4 = motion search, "
            "5 = P-picture depth ranges (fhevc_p_depth_range_device), 6 = first pass of the 4x4 PUs (fhevc_intra_first_pass_4x4*), "
            "7 = quarter-sample motion refinement (fhevc_motion_refine*), 8 = motion search of the rectangular PUs (fhevc_motion_search_pu*), "
            "9 = motion search of the PUs with a 4-sample side (fhevc_motion_search_pu_small*), 10 = quarter-sample refinement of the PUs "
            "(fhevc_motion_refine_pu*), 11 = the searches at HM's SearchRange (fhevc_motion_search_pu_wide*: one launch for nodes and PUs, one for the "
            "small PUs, each counted), 12 = the refinements at HM's SearchRange (fhevc_motion_refine_pu_wide*") in h


def test_python_mirror_matches_the_header():
    for sym in ARGS:
        assert sym in capi.SYMBOLS
    sig = inspect.signature(capi.Context.motion_refine_pu_wide)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "origin", "stride", "qp", "max_range", "nodes", "pus", "pus_small"]
    assert sig.parameters["max_range"].default == 64 and sig.parameters["qp"].default == 32 and sig.parameters["origin"].default == 0
    assert all(sig.parameters[k].default is None for k in ("stride", "nodes", "pus", "pus_small"))
    sig = inspect.signature(capi.Context.motion_refine_pu_wide_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_nodes", "d_out_nodes", "d_pus", "d_out_pus",
                                    "d_pus_small", "d_out_pus_small", "rows", "stream", "qp", "max_range"]
    assert all(sig.parameters[k].default is None for k in ("d_nodes", "d_out_nodes", "d_pus", "d_out_pus", "d_pus_small", "d_out_pus_small", "rows", "stream"))
    assert sig.parameters["max_range"].default == 64 and sig.parameters["qp"].default == 32
    assert "k_motion_refine.hip" in build.SOURCES and "k_motion_refine_pu.hip" in build.SOURCES


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, args in ARGS.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == len(args), sym
    # without a context both refuse before they touch a device
    assert lib.fhevc_motion_refine_pu_wide_device(None, None, 2, 64, 0, 2, 0, 1, 32, 64, None, None, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu_wide(None, None, None, 64, 32, 64, None, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 12, 0, None, None) == capi.E_INVALID
