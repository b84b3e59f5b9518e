"""The C-ABI surface of the coarse motion centres, of the integer searches around them and of their quarter-sample refinements (no GPU needed):
include/fasthevc.h declares the six entry points, states the definitions (the centres: no HM counterpart, the decimated grid, the candidates' cost,
coarse_range 1..14; the search and the refinement: vectors priced against the centre, ranges 1..8, centres within +-56; no state between calls), says what
is not covered, and documents timing slot 15; fasthevc_amd/capi.py mirrors it; the built library exports it; each entry point refuses a NULL context
before it touches a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

from fasthevc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fhevc_motion_centres_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                    "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int coarse_range",
                                    "fhevc_motion_node* d_centres", "void* stream"],
    "fhevc_motion_centres": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int coarse_range",
                             "fhevc_motion_node* centres"],
    "fhevc_motion_search_pu_centred_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                              "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int search_range",
                                              "const fhevc_motion_node* d_centres", "fhevc_motion_node* d_nodes", "fhevc_motion_node* d_pus",
                                              "fhevc_motion_node* d_pus_small", "void* stream"],
    "fhevc_motion_search_pu_centred": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int search_range",
                                       "const fhevc_motion_node* centres", "fhevc_motion_node* nodes", "fhevc_motion_node* pus", "fhevc_motion_node* pus_small"],
    "fhevc_motion_refine_pu_centred_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                              "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int max_range", "const fhevc_motion_node* d_centres",
                                              "const fhevc_motion_node* d_nodes", "fhevc_motion_qpel_node* d_out_nodes", "const fhevc_motion_node* d_pus",
                                              "fhevc_motion_qpel_node* d_out_pus", "const fhevc_motion_node* d_pus_small", "fhevc_motion_qpel_node* d_out_pus_small",
                                              "void* stream"],
    "fhevc_motion_refine_pu_centred": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int max_range",
                                       "const fhevc_motion_node* centres", "const fhevc_motion_node* nodes", "fhevc_motion_qpel_node* out_nodes",
                                       "const fhevc_motion_node* pus", "fhevc_motion_qpel_node* out_pus", "const fhevc_motion_node* pus_small",
                                       "fhevc_motion_qpel_node* out_pus_small"],
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
    for words in (r"NO HM counterpart", r"\(sum of the 4x4 samples at \(4X\.\., 4Y\.\.\) \+ 8\) >> 4", r"clamped to it", r"strict \"<\"",
                  r"\(16 \* sum over the counted cells of \|D_cur\(X, Y\) - D_ref\(X \+ dx, Y \+ dy\)\|\) >> \(bit_depth - 8\)",
                  r"c\[bits\(4 dx\) \+ bits\(4 dy\)\]", r"coarse_range is 1\.\.14", r"coarse_range outside 1\.\.14", r"keeps NO state between calls",
                  r"A CTU that owns no cell", r"Timed under slot 15", r"search_range outside 1\.\.8", r"satd_zero = the SAD AT THE CENTRE", r"outside \[-56, 56\]", r"NOT covered: search ranges above 8 around a centre",
                  r"c\[bits_q\(qx - 4 Px\) \+ bits_q\(qy - 4 Py\)\]", r"\|mvx - Px\|, \|mvy - Py\| <=\s+\*?\s*max_range", r"max_range outside 1\.\.8",
                  r"NOT covered: max_range above 8 around a centre", r"such a CTU is searched around \(0, 0\)"):
        assert re.search(words, h), words
    # fhevc_kernel_timing keeps slots 0..13 as they read and documents the new one
    assert re.search(r"13 = the partition-size selection \(fhevc_pu_shape_select_device\), 15 = the coarse motion centres \(fhevc_motion_centres\*\)", h)


def test_python_mirror_matches_the_header():
    for sym in ARGS:
        assert sym in capi.SYMBOLS
    sig = inspect.signature(capi.Context.motion_centres)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "origin", "stride", "qp", "coarse_range"]
    sig = inspect.signature(capi.Context.motion_centres_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_centres", "rows", "stream", "qp", "coarse_range"]
    assert all(sig.parameters[k].default is None for k in ("rows", "stream"))
    sig = inspect.signature(capi.Context.motion_search_pu_centred)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "centres", "origin", "stride", "qp", "search_range", "nodes", "pus", "pus_small"]
    sig = inspect.signature(capi.Context.motion_search_pu_centred_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_centres", "d_nodes", "d_pus", "d_pus_small", "rows",
                                    "stream", "qp", "search_range"]
    assert all(sig.parameters[k].default is None for k in ("d_nodes", "d_pus", "d_pus_small", "rows", "stream"))
    sig = inspect.signature(capi.Context.motion_refine_pu_centred)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "centres", "origin", "stride", "qp", "max_range", "nodes", "pus", "pus_small"]
    assert all(sig.parameters[k].default is None for k in ("nodes", "pus", "pus_small"))
    sig = inspect.signature(capi.Context.motion_refine_pu_centred_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_centres", "d_nodes", "d_out_nodes", "d_pus", "d_out_pus",
                                    "d_pus_small", "d_out_pus_small", "rows", "stream", "qp", "max_range"]
    assert all(sig.parameters[k].default is None for k in ("d_nodes", "d_out_nodes", "d_pus", "d_out_pus", "d_pus_small", "d_out_pus_small", "rows", "stream"))
    assert "k_motion_coarse.hip" in build.SOURCES
    assert capi.MOTION_DTYPE.itemsize == 16       # fhevc_motion_node: one entry per CTU


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, args in ARGS.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == len(args), sym
        # the ctypes type of every argument against the header's: pointers as void pointers, long long, int
        for t, a in zip(getattr(lib, sym).argtypes, args):
            want = C.c_void_p if "*" in a else C.c_longlong if a.startswith("long long") else C.c_int
            assert t is want, (sym, a, t)
    # without a context both refuse before they touch a device; so does the timing query, whatever the slot
    assert lib.fhevc_motion_centres_device(None, None, 2, 64, 0, 2, 0, 1, 32, 14, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_centres(None, None, None, 64, 32, 14, None) == capi.E_INVALID
    assert lib.fhevc_motion_search_pu_centred_device(None, None, 2, 64, 0, 2, 0, 1, 32, 8, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_search_pu_centred(None, None, None, 64, 32, 8, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu_centred_device(None, None, 2, 64, 0, 2, 0, 1, 32, 8, None, None, None, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu_centred(None, None, None, 64, 32, 8, None, None, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 15, 0, None, None) == capi.E_INVALID
    assert C.sizeof(C.c_uint32) * 3 + C.sizeof(C.c_int16) * 2 == 16
