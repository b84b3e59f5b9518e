"""The C-ABI surface of the PU motion search at HM's SearchRange (no GPU needed): include/fasthevc.h declares fhevc_motion_search_pu_wide and
fhevc_motion_search_pu_wide_device, states the definition (always SAD, ranges 1..64, no state between calls, the bit-count form of the vector
cost) and documents timing slot 11; the comments of the two PU searches point to the new entry point; fasthevc_amd/capi.py mirrors it; the built
library exports it; each entry point refuses a NULL context before it touches a device.  The bit-count form of the vector cost is checked against
the window's table (the oracle's fho_mv_cost, which the existing searches are pinned to) for every QP at R = 64."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np

from fasthevc_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fhevc_motion_search_pu_wide_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                           "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int search_range",
                                           "fhevc_motion_node* d_nodes", "fhevc_motion_node* d_pus", "fhevc_motion_node* d_pus_small", "void* stream"],
    "fhevc_motion_search_pu_wide": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int search_range",
                                    "fhevc_motion_node* nodes", "fhevc_motion_node* pus", "fhevc_motion_node* pus_small"],
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
    for words in (r"search_range 1\.\.64", r"ALWAYS SAD, whatever fhevc_set_motion_distortion says", r"NO state is kept between\s+\*?\s*calls",
                  r"2 floor\(log2 t\) \+ 1", r"t = v <= 0 \? \(-v << 3\) \+ 1 : v << 3", r"all three outputs null", r"search_range outside 1\.\.64"):
        assert re.search(words, h), words
    # the comments of the two PU searches name the entry point that has the ranges they leave out
    assert re.search(r"search ranges above 8 -- those are fhevc_motion_search_pu_wide's, further below", h)
    assert re.search(r"The ranges above 8 are fhevc_motion_search_pu_wide's, below, in SAD mode", h)
    # fhevc_kernel_timing keeps slots 0..10 as they read and documents the new one
    assert re.search(r"10 = quarter-sample refinement of the PUs\s+\*?\s*\(fhevc_motion_refine_pu\*\), 11 = the searches at HM's SearchRange", h)


def test_python_mirror_matches_the_header():
    for sym in ARGS:
        assert sym in capi.SYMBOLS
    sig = inspect.signature(capi.Context.motion_search_pu_wide)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "origin", "stride", "qp", "search_range", "nodes", "pus", "pus_small"]
    sig = inspect.signature(capi.Context.motion_search_pu_wide_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_nodes", "d_pus", "d_pus_small", "rows", "stream",
                                    "qp", "search_range"]
    assert all(sig.parameters[k].default is None for k in ("d_nodes", "d_pus", "d_pus_small", "rows", "stream"))
    assert "k_motion_pu.hip" in build.SOURCES and "k_motion_pu_small.hip" in build.SOURCES


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, args in ARGS.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == len(args), sym
    # without a context both refuse before they touch a device; slot 11 is known (the refusal is the NULL context's: slot 12 is refused with one too)
    assert lib.fhevc_motion_search_pu_wide_device(None, None, 2, 64, 0, 2, 0, 1, 32, 64, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_search_pu_wide(None, None, None, 64, 32, 64, None, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 11, 0, None, None) == capi.E_INVALID


def test_bit_count_form_of_the_vector_cost_equals_the_window_table(oracle):
    """what the MR = 64 kernels compute per vector -- the cost of (bits of dx + bits of dy) with bits(v) = 2 floor(log2 t) + 1,
    t = v <= 0 ? (-v << 3) + 1 : v << 3, cost(b) = HM's getCost(b) as fhevc_motion_refine tabulates it -- against getCostOfVectorWithPredictor of
    every vector of the +-64 window (oracle.fho_mv_cost, what mv_window_costs tabulates), for every QP"""
    def bits(v):
        t = ((-v) << 3) + 1 if v <= 0 else v << 3
        return 2 * (t.bit_length() - 1) + 1

    comp = np.array([bits(v) for v in range(-64, 65)])
    assert comp.max() == 19 and 2 * comp.max() < 40 and bits(0) == 1 and bits(1) == 7 and bits(-1) == 7 and bits(64) == 19 and bits(-64) == 19
    for qp in range(52):
        sl = math.sqrt(oracle.fho_lambda_intra(qp, 8))
        # getCost(b) = floor(motion lambda * b / 65536) with motion lambda = 65536 sqrt(lambda), in doubles: one component pair per number of bits
        per_bits = {}
        for dy in (-64, -1, 0, 1, 5, 64):
            for dx in range(-64, 65):
                per_bits.setdefault(bits(dx) + bits(dy), set()).add(oracle.fho_mv_cost(dx, dy, C.c_double(sl)))
        assert all(len(v) == 1 for v in per_bits.values()), qp     # the cost depends on the number of bits only
        table = {b: int((65536.0 * sl * b) / 65536.0) for b in range(40)}
        assert all(table[b] == next(iter(v)) for b, v in per_bits.items()), qp
    # ... and the whole window at three QPs
    for qp in (0, 32, 51):
        sl = math.sqrt(oracle.fho_lambda_intra(qp, 8))
        table = [int((65536.0 * sl * b) / 65536.0) for b in range(40)]
        for dy in range(-64, 65):
            for dx in range(-64, 65):
                assert table[comp[dx + 64] + comp[dy + 64]] == oracle.fho_mv_cost(dx, dy, C.c_double(sl)), (qp, dx, dy)
