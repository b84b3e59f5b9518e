"""The C-ABI surface of the motion search of the rectangular PUs (no GPU needed): include/fasthevc.h declares fhevc_motion_search_pu,
fhevc_motion_search_pu_device, fhevc_motion_pu_index and FHEVC_PUS_PER_CTU and documents timing slot 8 next to slots 0..7 as they read;
fasthevc_amd/capi.py mirrors them; the built library exports them; each entry point refuses a NULL context before it touches a device."""
import inspect
import os
import re
import subprocess

from fasthevc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fhevc_motion_search_pu_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                      "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int search_range",
                                      "fhevc_motion_node* d_nodes", "fhevc_motion_node* d_pus", "void* stream"],
    "fhevc_motion_search_pu": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int search_range",
                               "fhevc_motion_node* nodes", "fhevc_motion_node* pus"],
    "fhevc_motion_pu_index": ["int node", "int shape", "int part"],
}


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def test_header_declares_the_entry_points_and_the_count():
    h = _header()
    for sym, args in ARGS.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m, sym
        got = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert len(got) == len(args), (sym, got)
        for g, a in zip(got, args):
            assert g == a or (a == "fhevc_ctx*" and re.fullmatch(r"fhevc_ctx\s*\*\s*\w*", g)), (sym, g, a)
    assert re.search(r"#define\s+FHEVC_PUS_PER_CTU\s+124\b", h)
    # what the header leaves out on purpose is stated there
    for words in (r"AMP of 16x16 CUs", r"8x4 and 4x8 PUs", r"search ranges above 8", r"predictor other than zero"):
        assert re.search(words, h), words
    # fhevc_kernel_timing keeps slots 0..7 as they read and documents the new one
    assert re.search(r"0 = depth CNN, 1 = source Hadamard, 2 = first pass, 3 = pre-analysis, 4 = motion search,\s*\*?\s*5 = P-picture depth ranges", h)
    assert re.search(r"6 = first pass of the 4x4 PUs", h) and re.search(r"7 = quarter-sample motion refinement", h)
    assert re.search(r"8 = motion search of the rectangular PUs", h)


def test_python_mirror_matches_the_header():
    for sym in ARGS:
        assert sym in capi.SYMBOLS
    assert capi.PUS_PER_CTU == 124 and capi.MOTION_DTYPE.itemsize == 16
    assert capi.motion_pu_index(0, 0, 0) == 0 and capi.motion_pu_index(4, 5, 1) == 59 and capi.motion_pu_index(5, 0, 0) == 60
    assert capi.motion_pu_index(20, 1, 1) == 123 and capi.motion_pu_index(5, 2, 0) == -1 and capi.motion_pu_index(21, 0, 0) == -1
    sig = inspect.signature(capi.Context.motion_search_pu)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "origin", "stride", "qp", "search_range", "with_nodes"]
    assert sig.parameters["with_nodes"].default is False
    sig = inspect.signature(capi.Context.motion_search_pu_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_pus", "d_nodes", "rows", "stream", "qp",
                                    "search_range"]
    assert sig.parameters["d_nodes"].default is None and sig.parameters["rows"].default is None and sig.parameters["stream"].default is None
    assert "k_motion_pu.hip" in build.SOURCES


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, args in ARGS.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == len(args), sym
    # without a context both refuse before they touch a device; the timing slot is known; the index map needs no context
    assert lib.fhevc_motion_search_pu_device(None, None, 2, 64, 0, 2, 0, 1, 32, 4, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_search_pu(None, None, None, 64, 32, 4, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 8, 0, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_pu_index(1, 3, 1) == 19 and lib.fhevc_motion_pu_index(21, 0, 0) == -1
