"""The C-ABI surface of the quarter-sample motion refinement (no GPU needed): include/fasthevc.h declares fhevc_motion_refine,
fhevc_motion_refine_device and the 16-byte fhevc_motion_qpel_node, documents timing slot 7; fasthevc_amd/capi.py mirrors them; the built
library exports them; each refuses a NULL context before it touches a device."""
import inspect
import os
import re
import subprocess

from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fhevc_motion_refine_device": ["fhevc_ctx*", "const void* d_luma", "int sample_bytes", "int stride_samples", "long long frame_stride_samples",
                                   "int num_frames", "int ctu_row_begin", "int ctu_row_end", "int qp", "int max_range",
                                   "const fhevc_motion_node* d_nodes", "fhevc_motion_qpel_node* d_out", "void* stream"],
    "fhevc_motion_refine": ["fhevc_ctx*", "const int16_t* cur_luma", "const int16_t* ref_luma", "int stride_samples", "int qp", "int max_range",
                            "const fhevc_motion_node* nodes", "fhevc_motion_qpel_node* out"],
}


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def test_header_declares_the_entry_points_and_the_struct():
    h = _header()
    for sym, args in ARGS.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m, sym
        got = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
        assert len(got) == len(args), (sym, got)
        for g, a in zip(got, args):
            assert g == a or (a == "fhevc_ctx*" and re.fullmatch(r"fhevc_ctx\s*\*\s*\w*", g)), (sym, g, a)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fhevc_motion_qpel_node\s*;", h)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t satd_int", "uint32_t satd_best", "uint32_t cost_best", "int16_t mvx, mvy"]
    # fhevc_kernel_timing keeps slots 0..6 as they read and documents the new one
    assert re.search(r"0 = depth CNN, 1 = source Hadamard, 2 = first pass, 3 = pre-analysis, 4 = motion search,\s*\*?\s*5 = P-picture depth ranges", h)
    assert re.search(r"6 = first pass of the 4x4 PUs", h) and re.search(r"7 = quarter-sample motion refinement", h)


def test_python_mirror_matches_the_header():
    for sym in ARGS:
        assert sym in capi.SYMBOLS
    d = capi.MOTION_QPEL_DTYPE
    assert d.itemsize == 16 and d.names == ("satd_int", "satd_best", "cost_best", "mvx", "mvy")
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 12, 14]
    assert [d.fields[n][0].str for n in d.names] == ["<u4", "<u4", "<u4", "<i2", "<i2"]
    # the input struct it sits beside: same size, the vector at the same offsets
    assert capi.MOTION_DTYPE.itemsize == 16 and [capi.MOTION_DTYPE.fields[n][1] for n in ("mvx", "mvy")] == [12, 14]
    sig = inspect.signature(capi.Context.motion_refine)
    assert list(sig.parameters) == ["self", "cur_plane", "ref_plane", "nodes", "origin", "stride", "qp", "max_range"]
    sig = inspect.signature(capi.Context.motion_refine_device)
    assert list(sig.parameters) == ["self", "d_luma", "sample_bytes", "stride", "frame_stride", "num_frames", "d_nodes", "d_out", "rows", "stream", "qp",
                                    "max_range"]
    assert sig.parameters["rows"].default is None and sig.parameters["stream"].default is None and sig.parameters["qp"].default == 32


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, args in ARGS.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == len(args), sym
    # without a context both refuse before they touch a device; the timing slot is known
    assert lib.fhevc_motion_refine_device(None, None, 2, 64, 0, 2, 0, 1, 32, 4, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine(None, None, None, 64, 32, 4, None, None) == capi.E_INVALID
    assert lib.fhevc_kernel_timing(None, 7, 0, None, None) == capi.E_INVALID
