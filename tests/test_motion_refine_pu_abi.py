"""The C-ABI surface of the quarter-sample refinement of the PUs (no GPU needed): include/fasthevc.h declares fhevc_motion_refine_pu and
fhevc_motion_refine_pu_device, states both Hadamard branches and documents timing slot 10, and no longer lists the stage as left out;
fasthevc_amd/capi.py mirrors them; the built library exports them; each entry point refuses a NULL context before it touches a device."""
import inspect
import os
import re
import subprocess

from fasthevc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fhevc_motion_refine_pu_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                      "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int max_range",
                                      "const fhevc_motion_node* d_pus", "fhevc_motion_qpel_node* d_out_pus",
                                      "const fhevc_motion_node* d_pus_small", "fhevc_motion_qpel_node* d_out_pus_small", "void* stream"],
    "fhevc_motion_refine_pu": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int max_range",
                               "const fhevc_motion_node* pus", "fhevc_motion_qpel_node* out_pus",
                               "const fhevc_motion_node* pus_small", "fhevc_motion_qpel_node* out_pus_small"],
}


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def test_header_declares_the_entry_points_and_states_the_definition():
    h = _header()
    for sym, args in ARGS.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m, sym
        got = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert len(got) == len(args), (sym, got)
        for g, a in zip(got, args):
            assert g == a or (a == "fhevc_ctx*" and re.fullmatch(r"fhevc_ctx\s*\*\s*\w*", g)), (sym, g, a)
    flat = re.sub(r"\s*\n \*\s*", " ", h)     # comment lines joined
    for words in (r"xPatternSearchFracDIF behind the integer search, for every PU", r"\(sum \|H8 d H8\| \+ 2\) >> 2", r"\(sum \|H4 d H4\| \+ 1\) >> 1",
                  r"a 16x12 part is twelve 4x4 Hadamards", r"shifted ONCE by bit_depth - 8", r"s_acMvRefineH", r"s_acMvRefineQ",
                  r"Either family's in / out pair may be NULL together", r"max_range outside 1\.\.8", r"a pair with exactly one null member"):
        assert re.search(words, flat), words
    assert re.search(r"10 = quarter-sample refinement of the PUs", flat)
    # the stage is no longer listed as left out; what is still left out stays listed
    assert not re.search(r"quarter-sample refinement of PUs", flat)
    assert re.search(r"Still left out, on purpose: search ranges above 8, predictors other than zero\.", flat)


def test_python_mirror_matches_the_header():
    for sym in ARGS:
        assert sym in capi.SYMBOLS
    assert capi.MOTION_QPEL_DTYPE.itemsize == 16
    sig = inspect.signature(capi.Context.motion_refine_pu)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "origin", "stride", "qp", "max_range", "pus", "pus_small"]
    assert sig.parameters["pus"].default is None and sig.parameters["pus_small"].default is None
    sig = inspect.signature(capi.Context.motion_refine_pu_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_pus", "d_out_pus", "d_pus_small",
                                    "d_out_pus_small", "rows", "stream", "qp", "max_range"]
    assert sig.parameters["rows"].default is None and sig.parameters["stream"].default is None
    assert "k_motion_refine_pu.hip" in build.SOURCES


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, args in ARGS.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == len(args), sym
    # without a context both refuse before they touch a device; the timing slot is known
    assert lib.fhevc_motion_refine_pu_device(None, None, 2, 64, 0, 2, 0, 1, 32, 4, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu(None, None, None, 64, 32, 4, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 10, 0, None, None) == capi.E_INVALID
