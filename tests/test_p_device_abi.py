"""The C-ABI surface of the device-side P-picture decision (no GPU needed): include/fasthevc.h declares fhevc_p_depth_range_device,
fhevc_p_predict_frame and the three FHEVC_P_PREV_* constants, fasthevc_amd/capi.py mirrors them, the built library exports them."""
import ctypes as C
import inspect
import os
import re
import subprocess

from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fhevc_p_depth_range_device", "fhevc_p_predict_frame")


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def test_header_declares_the_entry_points_and_constants():
    h = _header()
    for sym in NEW:
        assert re.search(rf"\bint\s+{sym}\s*\(\s*fhevc_ctx\s*\*", h), sym
    values = {name: int(v) for name, v in re.findall(r"#define\s+FHEVC_P_PREV_([A-Z]+)\s+(\d+)", h)}
    assert values == {"COLOCATED": 0, "UNIT": 1, "NODE": 2}
    # the argument list the issue fixes: 12 and 11 parameters, the rule a const pointer, the stream last
    dev = re.search(r"fhevc_p_depth_range_device\s*\(([^;]*)\);", h).group(1)
    assert len(dev.split(",")) == 12 and "const fhevc_p_rule* rule" in dev and dev.strip().endswith("void* stream")
    host = re.search(r"fhevc_p_predict_frame\s*\(([^;]*)\);", h).group(1)
    assert len(host.split(",")) == 11 and "const uint8_t* prev_map" in host
    # fhevc_kernel_timing documents the new slot
    assert re.search(r"5 = P-picture depth ranges", h)


def test_python_mirror_matches_the_header():
    h = _header()
    for sym in NEW:
        assert sym in capi.SYMBOLS
    for name, v in re.findall(r"#define\s+FHEVC_P_PREV_([A-Z]+)\s+(\d+)", h):
        assert getattr(capi, f"P_PREV_{name}") == int(v)
    assert capi.P_PREV == {"colocated": capi.P_PREV_COLOCATED, "unit": capi.P_PREV_UNIT, "node": capi.P_PREV_NODE}
    sig = inspect.signature(capi.Context.p_depth_range_device)
    assert list(sig.parameters) == ["self", "d_nodes", "d_prev_maps", "num_pictures", "d_depth_min", "d_depth_max", "rows", "stream", "qp",
                                    "prev_mode", "rule"]
    assert sig.parameters["qp"].default == 32 and sig.parameters["prev_mode"].default == "colocated" and sig.parameters["d_depth_max"].default is None
    assert hasattr(capi.Context, "p_predict_frame")


def test_library_exports_the_entry_points():
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym in NEW:
        assert re.search(rf"\bT {sym}\b", exported), sym
    assert len(lib.fhevc_p_depth_range_device.argtypes) == 12 and len(lib.fhevc_p_predict_frame.argtypes) == 11
    # without a context both refuse before they touch a device
    rule = capi.p_rule_default()
    assert lib.fhevc_p_depth_range_device(None, None, None, 1, 0, 1, 32, 0, C.byref(rule), None, None, None) == capi.E_INVALID
    assert lib.fhevc_p_predict_frame(None, None, None, 64, 32, 4, None, 0, C.byref(rule), None, None) == capi.E_INVALID
