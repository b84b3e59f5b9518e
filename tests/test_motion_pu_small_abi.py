"""The C-ABI surface of the motion search of the PUs with a 4-sample side (no GPU needed): include/fasthevc.h declares
fhevc_motion_search_pu_small, fhevc_motion_search_pu_small_device, fhevc_motion_pu_small_index and FHEVC_PUS_SMALL_PER_CTU, states the 4x4-branch
fact and documents timing slot 9; fasthevc_amd/capi.py mirrors them; the built library exports them; each entry point refuses a NULL context
before it touches a device."""
import inspect
import os
import re
import subprocess

from fasthevc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fhevc_motion_search_pu_small_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                            "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int search_range",
                                            "fhevc_motion_node* d_pus", "void* stream"],
    "fhevc_motion_search_pu_small": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int search_range",
                                     "fhevc_motion_node* pus"],
    "fhevc_motion_pu_small_index": ["int node", "int shape", "int part"],
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
    assert re.search(r"#define\s+FHEVC_PUS_SMALL_PER_CTU\s+384\b", h)
    # the header's formula, evaluated: it is the layout capi implements
    m = re.search(r"entry \(k - 5\) \* 8 \+ \(shape - 2\) \* 2 \+ part", h)
    assert m and re.search(r"entry 128 \+ \(k - 21\) \* 4 \+ shape \* 2 \+ part", h)
    for k in range(5, 21):
        for shape in range(2, 6):
            for part in (0, 1):
                assert capi.motion_pu_small_index(k, shape, part) == (k - 5) * 8 + (shape - 2) * 2 + part
    for k in range(21, 85):
        for shape in range(2):
            for part in (0, 1):
                assert capi.motion_pu_small_index(k, shape, part) == 128 + (k - 21) * 4 + shape * 2 + part
    # the 4x4-branch fact and its consequence are stated; what is still left out is stated
    for words in (r"xCalcHADs4x4", r"twelve 4x4\s+\*?\s*Hadamards", r"NOT \"the node's SATD minus the\s+\*?\s*quarter\"", r"search ranges above 8",
                  r"predictors other than zero"):
        assert re.search(words, h), words
    assert re.search(r"9 = motion search of the PUs with a 4-sample side", h)


def test_python_mirror_matches_the_header():
    for sym in ARGS:
        assert sym in capi.SYMBOLS
    assert capi.PUS_SMALL_PER_CTU == 384 and capi.MOTION_DTYPE.itemsize == 16
    assert capi.motion_pu_small_index(5, 2, 0) == 0 and capi.motion_pu_small_index(20, 5, 1) == 127 and capi.motion_pu_small_index(21, 0, 0) == 128
    assert capi.motion_pu_small_index(84, 1, 1) == 383
    for bad in ((4, 2, 0), (5, 1, 0), (5, 6, 0), (21, 2, 0), (85, 0, 0), (0, 0, 0), (21, -1, 0), (21, 0, 2), (5, 2, -1)):
        assert capi.motion_pu_small_index(*bad) == -1, bad
    sig = inspect.signature(capi.Context.motion_search_pu_small)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "origin", "stride", "qp", "search_range"]
    sig = inspect.signature(capi.Context.motion_search_pu_small_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_pus", "rows", "stream", "qp", "search_range"]
    assert sig.parameters["rows"].default is None and sig.parameters["stream"].default is None
    assert "k_motion_pu_small.hip" in build.SOURCES


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, args in ARGS.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == len(args), sym
    # without a context both refuse before they touch a device; the timing slot is known; the index map needs no context
    assert lib.fhevc_motion_search_pu_small_device(None, None, 2, 64, 0, 2, 0, 1, 32, 4, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_search_pu_small(None, None, None, 64, 32, 4, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 9, 0, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_pu_small_index(5, 3, 1) == 3 and lib.fhevc_motion_pu_small_index(22, 1, 0) == 134 and lib.fhevc_motion_pu_small_index(4, 2, 0) == -1
