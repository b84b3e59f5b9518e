"""The C-ABI surface of the 4x4 first pass and of the device-side candidate lists (no GPU needed): include/fasthevc.h declares the four entry
points with their argument lists and FHEVC_PUS4_PER_CTU, documents timing slot 6; fasthevc_amd/capi.py mirrors them; the built library exports
them; each refuses a NULL context before it touches a device."""
import inspect
import os
import re
import subprocess

from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples", "int num_frames",
         "int ctu_row_begin", "int ctu_row_end", "int qp", "int num_candidates"]
ARGS = {
    "fhevc_intra_first_pass_4x4": ["fhevc_ctx*", "const int16_t* luma", "int stride_samples", "int qp", "int num_candidates", "fhevc_node_cost* best",
                                   "uint8_t* modes"],
    "fhevc_intra_first_pass_4x4_all": ["fhevc_ctx*", "const int16_t* luma", "int stride_samples", "int qp", "fhevc_node_cost* all"],
    "fhevc_intra_first_pass_4x4_device": BATCH + ["fhevc_node_cost* d_best", "uint8_t* d_modes", "void* stream"],
    "fhevc_intra_first_pass_candidates_device": BATCH + ["uint8_t* d_modes", "void* stream"],
}


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def test_header_declares_the_entry_points():
    h = _header()
    assert re.search(r"#define\s+FHEVC_PUS4_PER_CTU\s+256\b", h)
    for sym, args in ARGS.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m, sym
        got = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert len(got) == len(args), (sym, got)
        for g, a in zip(got, args):
            # the type and, where the issue names it, the parameter's name (the context's name is free)
            assert g == a or (a == "fhevc_ctx*" and re.fullmatch(r"fhevc_ctx\s*\*\s*\w*", g)), (sym, g, a)
    # fhevc_kernel_timing keeps slots 0..5 as they read and documents the new one
    assert re.search(r"0 = depth CNN, 1 = source Hadamard, 2 = first pass, 3 = pre-analysis, 4 = motion search,\s*\*?\s*5 = P-picture depth ranges", h)
    assert re.search(r"6 = first pass of the 4x4 PUs", h)


def test_python_mirror_matches_the_header():
    assert capi.PUS4_PER_CTU == 256
    for sym in ARGS:
        assert sym in capi.SYMBOLS
    sig = inspect.signature(capi.Context.intra_first_pass_4x4)
    assert list(sig.parameters) == ["self", "plane", "origin", "stride", "qp", "num_candidates"]
    assert sig.parameters["qp"].default == 32 and sig.parameters["num_candidates"].default == 8
    assert list(inspect.signature(capi.Context.intra_first_pass_4x4_all).parameters) == ["self", "plane", "origin", "stride", "qp"]
    sig = inspect.signature(capi.Context.intra_first_pass_4x4_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_best", "d_modes", "rows", "stream", "qp",
                                    "num_candidates"]
    assert sig.parameters["d_best"].default is None and sig.parameters["d_modes"].default is None and sig.parameters["num_candidates"].default == 8
    sig = inspect.signature(capi.Context.intra_first_pass_candidates_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_modes", "rows", "stream", "qp",
                                    "num_candidates"]


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, args in ARGS.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == len(args), sym
    # without a context every one of them refuses before it touches a device
    assert lib.fhevc_intra_first_pass_4x4(None, None, 64, 32, 8, None, None) == capi.E_INVALID
    assert lib.fhevc_intra_first_pass_4x4_all(None, None, 64, 32, None) == capi.E_INVALID
    assert lib.fhevc_intra_first_pass_4x4_device(None, None, 2, 64, 0, 1, 0, 1, 32, 8, None, None, None) == capi.E_INVALID
    assert lib.fhevc_intra_first_pass_candidates_device(None, None, 2, 64, 0, 1, 0, 1, 32, 8, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 6, 0, None, None) == capi.E_INVALID
