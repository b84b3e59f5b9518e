"""ctypes mirror of include/fasthevc.h -- the host-side view of the C ABI used by tests, the trainer and bench.py.

There is no fallback: if the HIP library is missing or no gfx950 device is usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import weights as _weights

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libfasthevc_hip.so")

OK, E_INVALID, E_NO_DEVICE, E_HIP, E_WEIGHTS, E_NOMEM, E_STATE = 0, -1, -2, -3, -4, -5, -6
BACKEND_HIP = 1
NODES_PER_CTU = 85
PUS4_PER_CTU = 256  # 4x4 PUs of a CTU, raster 16x16: the depth map's unit order
LOGITS_PER_CTU = 42
PUS_SMALL_PER_CTU = 384  # PUs with a 4-sample side: AMP of the 16x16 nodes, 8x4 / 4x8 of the 8x8 nodes (FHEVC_PUS_SMALL_PER_CTU; order: motion_pu_small_index)
PUS_PER_CTU = 124  # rectangular PUs of a CTU whose sides are multiples of 8 (FHEVC_PUS_PER_CTU; order: motion_pu_index)

# every symbol include/fasthevc.h declares (tests/test_host_logic.py::test_c_abi_exports_every_declared_symbol checks header <-> this list <-> the .so)
SYMBOLS = [
    "fhevc_create", "fhevc_destroy", "fhevc_set_weights", "fhevc_predict_frame", "fhevc_satd",
    "fhevc_intra_first_pass", "fhevc_predict_frames_device", "fhevc_band", "fhevc_kernel_timing",
    "fhevc_enable_kernel_timing", "fhevc_get_stats", "fhevc_last_error", "fhevc_version",
    "fhevc_expand_depth_flags_device", "fhevc_aq_parts", "fhevc_preanalyze", "fhevc_preanalyze_frames_device", "fhevc_aq_qp", "fhevc_intra_first_pass_device",
    "fhevc_predict_frame_range", "fhevc_predict_frames_device_range",
    "fhevc_motion_search", "fhevc_motion_search_device", "fhevc_intra_first_pass_all", "fhevc_intra_first_pass_candidates", "fhevc_p_rule_default", "fhevc_p_rule_default_wide", "fhevc_p_depth_range", "fhevc_p_motion_compensated_depth", "fhevc_p_node_depth",
    "fhevc_predict_frames", "fhevc_alloc_host", "fhevc_free_host", "fhevc_set_cnn_arith", "fhevc_get_cnn_arith", "fhevc_set_motion_distortion", "fhevc_read_yuv_luma",
    "fhevc_p_depth_range_device", "fhevc_p_predict_frame",
    "fhevc_intra_first_pass_4x4", "fhevc_intra_first_pass_4x4_all", "fhevc_intra_first_pass_4x4_device", "fhevc_intra_first_pass_candidates_device",
    "fhevc_motion_refine", "fhevc_motion_refine_device",
    "fhevc_motion_search_pu", "fhevc_motion_search_pu_device", "fhevc_motion_pu_index",
    "fhevc_motion_search_pu_small", "fhevc_motion_search_pu_small_device", "fhevc_motion_pu_small_index",
    "fhevc_motion_refine_pu", "fhevc_motion_refine_pu_device",
    "fhevc_motion_search_pu_wide", "fhevc_motion_search_pu_wide_device",
    "fhevc_motion_refine_pu_wide", "fhevc_motion_refine_pu_wide_device",
    "fhevc_pu_shape_rule_default", "fhevc_pu_shape_select", "fhevc_pu_shape_select_device", "fhevc_p_shape_frame",
    "fhevc_motion_centres", "fhevc_motion_centres_device", "fhevc_motion_search_pu_centred", "fhevc_motion_search_pu_centred_device",
    "fhevc_motion_refine_pu_centred", "fhevc_motion_refine_pu_centred_device",
    "fhevc_p_tree_rule_default", "fhevc_p_tree_select", "fhevc_p_tree_select_device", "fhevc_p_tree_frame",
    "fhevc_motion_merge", "fhevc_motion_merge_device", "fhevc_p_tree_select_merge", "fhevc_p_tree_select_merge_device", "fhevc_p_tree_merge_frame",
    "fhevc_motion_merge_pu", "fhevc_motion_merge_pu_device", "fhevc_pu_shape_select_merge", "fhevc_pu_shape_select_merge_device", "fhevc_p_tree_merge_pu_frame",
    "fhevc_motion_skip", "fhevc_motion_skip_device", "fhevc_p_tree_select_skip", "fhevc_p_tree_select_skip_device",
    "fhevc_motion_amvp", "fhevc_motion_amvp_device", "fhevc_motion_amvp_picture", "fhevc_p_tree_amvp_frame",
    "fhevc_intra_p", "fhevc_intra_p_device", "fhevc_intra_p_picture", "fhevc_p_tree_select_intra", "fhevc_p_tree_select_intra_device", "fhevc_p_tree_intra_frame",
    "fhevc_motion_rd", "fhevc_motion_rd_device", "fhevc_motion_rd_lambda_q8", "fhevc_p_tree_select_rd", "fhevc_p_tree_select_rd_device",
    "fhevc_motion_rd_pu", "fhevc_motion_rd_pu_device", "fhevc_p_tree_select_rd_pu", "fhevc_p_tree_select_rd_pu_device", "fhevc_p_tree_rd_frame",
    "fhevc_intra_rd", "fhevc_intra_rd_device", "fhevc_p_tree_rd_intra_frame",
    "fhevc_motion_rd_qt", "fhevc_motion_rd_qt_device", "fhevc_motion_rd_pu_qt", "fhevc_motion_rd_pu_qt_device", "fhevc_p_tree_rd_qt_frame",
    "fhevc_intra_rd_qt", "fhevc_intra_rd_qt_device", "fhevc_p_tree_rd_intra_qt_frame",
    "fhevc_intra_rd_nxn", "fhevc_intra_rd_nxn_device", "fhevc_p_tree_rd_intra_nxn_frame",
    "fhevc_intra_search_rule_default", "fhevc_intra_rd_search", "fhevc_intra_rd_search_device", "fhevc_p_tree_rd_intra_search_frame",
]
CNN_ARITH = {"i8": 8, "f16": 16}
# where fhevc_p_depth_range_device / fhevc_p_predict_frame take the reference picture's depths from (FHEVC_P_PREV_*)
P_PREV_COLOCATED, P_PREV_UNIT, P_PREV_NODE = 0, 1, 2
P_PREV = {"colocated": P_PREV_COLOCATED, "unit": P_PREV_UNIT, "node": P_PREV_NODE}
# partition sizes of fhevc_pu_shape_select*: HM's PartSize numbers (FHEVC_PART_*; 3, NxN, is never produced)
PART_2Nx2N, PART_2NxN, PART_Nx2N, PART_2NxnU, PART_2NxnD, PART_nLx2N, PART_nRx2N = 0, 1, 2, 4, 5, 6, 7


class Cfg(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("bit_depth", C.c_int), ("ctu_size", C.c_int),
                ("max_depth", C.c_int), ("num_devices", C.c_int), ("device_ids", C.POINTER(C.c_int)),
                ("weights_path", C.c_char_p), ("backend", C.c_int), ("max_frames", C.c_int)]


class PRule(C.Structure):
    _fields_ = [("w", (C.c_int32 * 10) * 3), ("t_split", C.c_int32 * 3), ("t_stop", C.c_int32 * 3), ("window", C.c_int32)]


class PuShapeRule(C.Structure):
    """fhevc_pu_shape_rule: margins per level (64, 32, 16, 8) and the AMP gate"""
    _fields_ = [("margin_q8", C.c_int32 * 4), ("margin_abs", C.c_int32 * 4), ("amp_mode", C.c_int32)]


class IntraSearchRule(C.Structure):
    """fhevc_intra_search_rule: list entries read per node of level 0..3 and per 4x4 PU, whether planar is appended; 8 bytes"""
    _fields_ = [("count", C.c_uint8 * 4), ("count4", C.c_uint8), ("append_planar", C.c_uint8), ("pad", C.c_uint8 * 2)]


# ... and the same eight bytes as a record
INTRA_SEARCH_RULE_DTYPE = np.dtype([("count", np.uint8, (4,)), ("count4", np.uint8), ("append_planar", np.uint8), ("pad", np.uint8, (2,))])


class PTreeRule(C.Structure):
    """fhevc_p_tree_rule: the margins of the two decisions and the split cost per level (64, 32, 16)"""
    _fields_ = [("split_q8", C.c_int32 * 3), ("split_abs", C.c_int32 * 3), ("stop_q8", C.c_int32 * 3), ("stop_abs", C.c_int32 * 3), ("split_cost", C.c_int32 * 3)]


class MotionRdPuInputs(C.Structure):
    """fhevc_motion_rd_pu_inputs: ten pointers (device or host), None for an array left out"""
    _fields_ = [(n, C.c_void_p) for n in ("nodes", "pus", "pus_small", "merge_pus", "merge_pus_small", "mvp_nodes", "mvp_pus", "mvp_pus_small", "shapes", "fold")]


class NodeCost(C.Structure):
    _fields_ = [("satd", C.c_uint32), ("mode", C.c_uint32), ("cost", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("ctus", C.c_uint64), ("bytes_h2d", C.c_uint64), ("bytes_d2h", C.c_uint64),
                ("kernels_launched", C.c_uint64), ("ms_h2d", C.c_double), ("ms_kernels", C.c_double),
                ("ms_d2h", C.c_double), ("last_cnn_ms", C.c_double), ("last_hadamard_ms", C.c_double),
                ("last_first_pass_ms", C.c_double), ("devices", C.c_uint64), ("devices_failed", C.c_uint64)]


NODE_DTYPE = np.dtype([("satd", np.uint32), ("mode", np.uint32), ("cost", np.float64)])
MOTION_DTYPE = np.dtype([("satd_zero", np.uint32), ("satd_best", np.uint32), ("cost_best", np.uint32), ("mvx", np.int16), ("mvy", np.int16)])
# fhevc_motion_qpel_node: the vector in QUARTER samples
MOTION_QPEL_DTYPE = np.dtype([("satd_int", np.uint32), ("satd_best", np.uint32), ("cost_best", np.uint32), ("mvx", np.int16), ("mvy", np.int16)])
# fhevc_pu_shape_node: one record per CU node
SHAPE_DTYPE = np.dtype([("cost_2Nx2N", np.uint32), ("cost_best", np.uint32), ("cost_second", np.uint32), ("best", np.uint8), ("second", np.uint8),
                        ("mask", np.uint8), ("avail", np.uint8)])

# fhevc_motion_merge_node: the cheapest merge candidate of a CU node (src: 0..4 = L, A, AR, BL, AL, 5 = the zero vector; idx / num: its place in / the length of the list)
MOTION_MERGE_DTYPE = np.dtype([("satd_best", np.uint32), ("cost_best", np.uint32), ("mvx", np.int16), ("mvy", np.int16), ("idx", np.uint8), ("num", np.uint8),
                               ("src", np.uint8), ("pad", np.uint8)])
# fhevc_motion_skip_node: the transformed and quantised residual of a CU node at its merge vector (flags: SKIP_ZERO_PLAIN under the P-slice dead zone,
# SKIP_ZERO_HALF under the rounding RDOQ starts from)
MOTION_SKIP_DTYPE = np.dtype([("coef_max", np.uint32), ("level_sum", np.uint32), ("nonzero", np.uint16), ("flags", np.uint8), ("pad", np.uint8),
                              ("mvx", np.int16), ("mvy", np.int16)])
SKIP_ZERO_PLAIN, SKIP_ZERO_HALF = 1, 2
# fhevc_motion_rd_node: the RD estimate of a CU node at a vector (flags: the skip record's two bits, RD_TU_SPLIT: some depth-0 TU is split).  cost_rd lies
# where the merge and the selection records keep cost_best, flags where the skip record keeps flags
MOTION_RD_DTYPE = np.dtype([("dist", np.uint32), ("cost_rd", np.uint32), ("bits", np.uint16), ("flags", np.uint8), ("tu_split", np.uint8),
                            ("mvx", np.int16), ("mvy", np.int16)])
RD_SOURCE_MERGE, RD_SOURCE_EXPLICIT = 0, 1
# fhevc_motion_rd_pu_node: the RD estimate of a CU node under one of HM's partition sizes; bytes 0..11 are MOTION_RD_DTYPE's (part: the PartSize priced, 255 in a
# marker; merged bit i: part i took its merge vector)
MOTION_RD_PU_DTYPE = np.dtype([("dist", np.uint32), ("cost_rd", np.uint32), ("bits", np.uint16), ("flags", np.uint8), ("tu_split", np.uint8),
                               ("part", np.uint8), ("merged", np.uint8), ("pad", np.uint8, (2,))])
# part_mode of fhevc_motion_rd_pu*: a PART_* number for every node, or the selection's best / second size per node
RD_PART_BEST, RD_PART_SECOND = 8, 9
# part of a record of fhevc_intra_rd*: the intra candidate (FHEVC_RD_PART_INTRA); its mode lies in pad[0]
RD_PART_INTRA = 16
# ... and the NxN candidate of an 8x8 node (FHEVC_RD_PART_INTRA_NXN): four 4x4 PUs at the four modes of the 4x4 first pass, tu_split 1, pad zero
RD_PART_INTRA_NXN = 17
# fhevc_intra_rd_nxn_node: the plain NxN candidate of an 8x8 node (cbf bit i: TU i has a non-zero level; the marker: 0xFF everywhere but flags = cbf = 0)
INTRA_RD_NXN_DTYPE = np.dtype([("dist", np.uint32), ("cost_rd", np.uint32), ("bits", np.uint16), ("flags", np.uint8), ("cbf", np.uint8), ("modes", np.uint8, (4,))])
NXN_PER_CTU = 64
RD_TU_SPLIT = 4
# fhevc_motion_mvp: the predictor fhevc_motion_amvp* priced an entry against (src: 0..4 = L, A, AR, BL, AL, 5 = a filled zero; idx = src = 255: no price)
MOTION_MVP_DTYPE = np.dtype([("px", np.int16), ("py", np.int16), ("idx", np.uint8), ("num_spatial", np.uint8), ("src", np.uint8), ("bits", np.uint8)])
MVP_BIT_COSTS = 67
MERGE_L, MERGE_A, MERGE_AR, MERGE_BL, MERGE_AL, MERGE_ZERO = 0, 1, 2, 3, 4, 5
# fhevc_p_tree_node: one record per CU node (flags: 1 split_sure, 2 stop_sure, 4 CROSSING, 8 ABSENT, 16 own available, 32 kids available)
TREE_DTYPE = np.dtype([("cost_own", np.uint32), ("cost_kids", np.uint32), ("cost_tree", np.uint32), ("flags", np.uint8), ("level", np.uint8), ("pad", np.uint8, (2,))])
# fhevc_intra_p_node: the intra candidate of a CU node of a P picture (part 0: 2Nx2N, modes = the mode four times; part 1: NxN, the modes of the four PUs)
INTRA_P_DTYPE = np.dtype([("satd_best", np.uint32), ("cost_best", np.uint32), ("modes", np.uint8, (4,)), ("part", np.uint8), ("pad", np.uint8, (3,))])
TREE_INTRA = 1  # bit 0 of pad[0] (byte 14) of a tree record of fhevc_p_tree_select_intra*: own is the intra cost


def motion_pu_index(node, shape, part):
    """fhevc_motion_pu_index: the entry of a CTU's PUS_PER_CTU that holds `part` (0, 1) of `shape` (0 2NxN, 1 Nx2N, 2 2NxnU, 3 2NxnD, 4 nLx2N, 5 nRx2N) of
    CU node `node`; -1 where the combination is not covered.  Pure arithmetic, the same as the library's."""
    if node < 0 or shape < 0 or part not in (0, 1):
        return -1
    if node < 5:
        return node * 12 + shape * 2 + part if shape < 6 else -1
    if node < 21:
        return 60 + (node - 5) * 4 + shape * 2 + part if shape < 2 else -1
    return -1


def motion_pu_small_index(node, shape, part):
    """fhevc_motion_pu_small_index: the entry of a CTU's PUS_SMALL_PER_CTU that holds `part` (0, 1) of `shape` (numbers of motion_pu_index) of CU node `node`:
    shapes 2..5 of the 16x16 nodes 5..20, then shapes 0..1 of the 8x8 nodes 21..84; -1 for anything else.  Pure arithmetic, the same as the library's."""
    if part not in (0, 1):
        return -1
    if 5 <= node < 21:
        return (node - 5) * 8 + (shape - 2) * 2 + part if 2 <= shape < 6 else -1
    if 21 <= node < 85:
        return 128 + (node - 21) * 4 + shape * 2 + part if 0 <= shape < 2 else -1
    return -1


class FastHevcError(RuntimeError):
    def __init__(self, code, text=""):
        super().__init__(f"fasthevc error {code}: {text}")
        self.code = code


_lib = None


def _share_the_hosts_hip_runtime():
    """A PyTorch wheel bundles its own libamdhip64.so with the SONAME of /opt/rocm's.  Whichever copy a process maps first
    serves every later DT_NEEDED of that SONAME, and torch's other bundled libraries only work with torch's copy: if this
    library came first (binding /opt/rocm's), a later `import torch` finds "No HIP GPUs".  So when torch is installed and not
    yet imported, map ITS runtime first (without importing torch); the in-tree library then shares it, in either order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return  # torch's runtime is already mapped
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return  # no torch in this interpreter (e.g. a plain C++ host): the system runtime is the only one
    rt = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(rt):
        C.CDLL(rt, mode=C.RTLD_GLOBAL)


def load_library(path=None):
    """dlopen the in-tree HIP library; raises if it has not been built (no silent fallback).  `path`: another build of the same
    library (tools/build_variant.sh), bound separately and not cached -- same-process A/B timing of kernel variants only."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib_path = path or LIB_PATH
    if not os.path.exists(lib_path):
        raise FileNotFoundError(f"{lib_path} not built: run `python -m fasthevc_amd.build` (or __graft_entry__.build())")
    _share_the_hosts_hip_runtime()
    lib = C.CDLL(lib_path)
    vp = C.c_void_p
    lib.fhevc_create.argtypes = [C.POINTER(vp), C.POINTER(Cfg)]
    lib.fhevc_destroy.argtypes = [vp]
    lib.fhevc_destroy.restype = None
    lib.fhevc_set_weights.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.fhevc_predict_frame.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_predict_frame_range.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_predict_frames_device_range.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.fhevc_satd.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
    lib.fhevc_intra_first_pass.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    lib.fhevc_intra_first_pass_all.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.fhevc_intra_first_pass_candidates.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.fhevc_intra_first_pass_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, vp, vp]
    lib.fhevc_intra_first_pass_4x4.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_intra_first_pass_4x4_all.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    lib.fhevc_intra_first_pass_4x4_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_intra_first_pass_candidates_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                                             C.c_int, C.c_int, vp, vp]
    lib.fhevc_predict_frames_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                                C.c_int, vp, vp, vp, vp, vp]
    lib.fhevc_expand_depth_flags_device.argtypes = [vp, vp, C.c_int, vp, vp]
    lib.fhevc_band.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.fhevc_aq_parts.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    lib.fhevc_preanalyze.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    lib.fhevc_aq_qp.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.fhevc_preanalyze_frames_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                                   C.c_int, vp, vp]
    lib.fhevc_set_cnn_arith.argtypes = [vp, C.c_int]
    lib.fhevc_set_motion_distortion.argtypes = [vp, C.c_int]
    lib.fhevc_read_yuv_luma.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                        C.c_longlong, C.c_longlong]
    lib.fhevc_get_cnn_arith.argtypes = [vp]
    lib.fhevc_motion_search.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.fhevc_motion_search_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_motion_refine.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_motion_refine_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_motion_search_pu.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_motion_search_pu_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_motion_pu_index.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.fhevc_motion_search_pu_small.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.fhevc_motion_search_pu_small_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_motion_pu_small_index.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.fhevc_motion_search_pu_wide.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_motion_search_pu_wide_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.fhevc_motion_refine_pu.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.fhevc_motion_refine_pu_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.fhevc_p_rule_default.argtypes = [C.POINTER(PRule)]
    lib.fhevc_p_rule_default.restype = None
    lib.fhevc_p_rule_default_wide.argtypes = [C.POINTER(PRule)]
    lib.fhevc_p_rule_default_wide.restype = None
    lib.fhevc_p_depth_range.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PRule), vp, vp]
    lib.fhevc_p_motion_compensated_depth.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.fhevc_p_node_depth.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.fhevc_p_depth_range_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PRule), vp, vp, vp]
    lib.fhevc_p_predict_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(PRule), vp, vp]
    lib.fhevc_pu_shape_rule_default.argtypes = [C.POINTER(PuShapeRule)]
    lib.fhevc_pu_shape_rule_default.restype = None
    lib.fhevc_pu_shape_select.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(PuShapeRule), vp, vp]
    lib.fhevc_pu_shape_select_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), vp, vp, vp]
    lib.fhevc_p_shape_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), vp]
    lib.fhevc_p_tree_rule_default.argtypes = [C.POINTER(PTreeRule)]
    lib.fhevc_p_tree_rule_default.restype = None
    lib.fhevc_p_tree_select.argtypes = [vp, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp]
    lib.fhevc_p_tree_select_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_p_tree_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), vp, vp, vp]
    lib.fhevc_motion_merge.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_motion_merge_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_p_tree_select_merge.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp]
    lib.fhevc_p_tree_select_merge_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_p_tree_merge_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_motion_merge_pu.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_motion_merge_pu_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.fhevc_pu_shape_select_merge.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(PuShapeRule), vp, vp, vp]
    lib.fhevc_pu_shape_select_merge_device.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), vp, vp, vp, vp]
    lib.fhevc_motion_skip.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_motion_skip_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_p_tree_select_skip.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp]
    lib.fhevc_p_tree_select_skip_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_motion_rd.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_motion_rd_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    if path is None or hasattr(lib, "fhevc_motion_rd_qt"):   # another build (A/B against the parent commit) may predate the entry points with tu_depths
        lib.fhevc_motion_rd_qt.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]
        lib.fhevc_motion_rd_qt_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]
        lib.fhevc_motion_rd_pu_qt.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MotionRdPuInputs), C.c_int, vp]
        lib.fhevc_motion_rd_pu_qt_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MotionRdPuInputs),
                                                     C.c_int, vp, vp]
        lib.fhevc_p_tree_rd_qt_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), C.c_int, C.c_int, vp, vp, vp, vp,
                                                 vp, vp]
    lib.fhevc_motion_rd_lambda_q8.argtypes = [C.c_int]
    lib.fhevc_motion_rd_lambda_q8.restype = C.c_uint32
    lib.fhevc_p_tree_select_rd.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp]
    lib.fhevc_p_tree_select_rd_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_p_tree_merge_pu_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_motion_amvp.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.fhevc_motion_amvp_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.fhevc_motion_amvp_picture.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.fhevc_p_tree_amvp_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_intra_p.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.fhevc_intra_p_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.fhevc_intra_p_picture.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.fhevc_p_tree_select_intra.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp]
    lib.fhevc_p_tree_select_intra_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_motion_rd_pu.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MotionRdPuInputs), vp]
    lib.fhevc_motion_rd_pu_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MotionRdPuInputs), vp, vp]
    lib.fhevc_p_tree_select_rd_pu.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp]
    lib.fhevc_p_tree_select_rd_pu_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PTreeRule), vp, vp, vp, vp]
    lib.fhevc_p_tree_rd_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), C.c_int, vp, vp, vp, vp, vp, vp]
    lib.fhevc_intra_rd.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]
    lib.fhevc_intra_rd_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp]
    lib.fhevc_p_tree_rd_intra_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), C.c_int, vp, vp, vp, vp, vp, vp, vp]
    if path is None or hasattr(lib, "fhevc_intra_rd_qt"):   # another build (A/B against the parent commit) may predate the intra entry points with tu_depths
        lib.fhevc_intra_rd_qt.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp]
        lib.fhevc_intra_rd_qt_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp]
        lib.fhevc_p_tree_rd_intra_qt_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), C.c_int, C.c_int, vp, vp, vp,
                                                       vp, vp, vp, vp]
    if path is None or hasattr(lib, "fhevc_intra_rd_nxn"):   # another build (A/B against the parent commit) may predate the entry points with the NxN candidate
        lib.fhevc_intra_rd_nxn.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp]
        lib.fhevc_intra_rd_nxn_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp]
        lib.fhevc_p_tree_rd_intra_nxn_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), C.c_int, vp, vp, vp,
                                                        vp, vp, vp, vp, vp]
    if path is None or hasattr(lib, "fhevc_intra_rd_search"):   # another build (A/B against the parent commit) may predate the candidate search
        lib.fhevc_intra_search_rule_default.argtypes = [C.POINTER(IntraSearchRule)]
        lib.fhevc_intra_search_rule_default.restype = None
        lib.fhevc_intra_rd_search.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(IntraSearchRule), vp, vp, C.c_int, vp, vp]
        lib.fhevc_intra_rd_search_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int,
                                                     C.POINTER(IntraSearchRule), vp, vp, C.c_int, vp, vp, vp]
        lib.fhevc_p_tree_rd_intra_search_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule),
                                                           C.POINTER(IntraSearchRule), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.fhevc_p_tree_intra_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PuShapeRule), C.POINTER(PTreeRule), C.c_int, vp, vp, vp, vp, vp]
    lib.fhevc_predict_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, vp, vp]
    lib.fhevc_alloc_host.argtypes = [vp, C.c_size_t]
    lib.fhevc_alloc_host.restype = vp
    lib.fhevc_free_host.argtypes = [vp, vp]
    lib.fhevc_free_host.restype = None
    lib.fhevc_motion_refine_pu_wide.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.fhevc_motion_refine_pu_wide_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.fhevc_motion_centres.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.fhevc_motion_centres_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.fhevc_motion_search_pu_centred.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.fhevc_motion_search_pu_centred_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.fhevc_motion_refine_pu_centred.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.fhevc_motion_refine_pu_centred_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.fhevc_kernel_timing.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.fhevc_enable_kernel_timing.argtypes = [vp, C.c_int]
    lib.fhevc_get_stats.argtypes = [vp, vp, C.c_size_t]
    lib.fhevc_last_error.argtypes = [vp]
    lib.fhevc_last_error.restype = C.c_char_p
    lib.fhevc_version.restype = C.c_char_p
    if path is None:
        _lib = lib
    return lib


def read_yuv_luma(path, file_size, file_bit_depth, out, first=0, internal_bit_depth=None, chroma_format=420):
    """The library's own luma reader (fhevc_read_yuv_luma, host C++): fills out [count, H, W] (uint8, or int16 Pel) -- e.g. pinned memory
    from Context.alloc_host -- with the luma planes of pictures first.. of a planar YUV file, padded by edge replication to out's
    H x W and shifted to the internal bit depth.  -> number of pictures read."""
    fw, fh = file_size
    count, H, W = out.shape
    assert out.dtype in (np.uint8, np.int16) and out.flags["C_CONTIGUOUS"]
    n = load_library().fhevc_read_yuv_luma(os.fsencode(path), fw, fh, file_bit_depth, chroma_format, first, count, W, H,
                                           internal_bit_depth or file_bit_depth, out.dtype.itemsize, out.ctypes.data, W, W * H)
    if n < 0:
        raise FastHevcError(n, "fhevc_read_yuv_luma")
    return n


def p_rule_default():
    r = PRule()
    load_library().fhevc_p_rule_default(C.byref(r))
    return r


def p_rule_default_wide():
    r = PRule()
    load_library().fhevc_p_rule_default_wide(C.byref(r))
    return r


def pu_shape_rule_default():
    r = PuShapeRule()
    load_library().fhevc_pu_shape_rule_default(C.byref(r))
    return r


def pu_shape_rule(margin_q8=0, margin_abs=0, amp_mode=1):
    """a PuShapeRule from scalars (the same margin at every level) or sequences of four"""
    q8 = [margin_q8] * 4 if np.isscalar(margin_q8) else list(margin_q8)
    ab = [margin_abs] * 4 if np.isscalar(margin_abs) else list(margin_abs)
    return PuShapeRule((C.c_int32 * 4)(*q8), (C.c_int32 * 4)(*ab), amp_mode)


def intra_search_rule_default():
    r = IntraSearchRule()
    load_library().fhevc_intra_search_rule_default(C.byref(r))
    return r


def intra_search_rule(count=(3, 3, 3, 8), count4=8, append_planar=1):
    r = IntraSearchRule()
    r.count[:] = list(count)
    r.count4, r.append_planar = count4, append_planar
    return r


def p_tree_rule_default():
    r = PTreeRule()
    load_library().fhevc_p_tree_rule_default(C.byref(r))
    return r


def p_tree_rule(split_q8=0, split_abs=0, stop_q8=0, stop_abs=0, split_cost=0):
    """a PTreeRule from scalars (the same value at every level) or sequences of three"""
    three = lambda v: (C.c_int32 * 3)(*([v] * 3 if np.isscalar(v) else list(v)))
    return PTreeRule(three(split_q8), three(split_abs), three(stop_q8), three(stop_abs), three(split_cost))


def p_tree_select(shapes, width, height, rule=None, with_tree=False):
    """config 4, host side: (depth_min, depth_max) [numCtus, 256] of a P picture from the selection's records [numCtus, 85] SHAPE_DTYPE (only cost_best is
    read), decided bottom-up over the quad-tree; with_tree: (depth_min, depth_max, records [numCtus, 85] TREE_DTYPE)"""
    lib = load_library()
    rule = rule if rule is not None else p_tree_rule_default()
    shapes = np.ascontiguousarray(shapes)
    assert shapes.dtype.itemsize == 16
    cw = (width + 63) // 64
    n = shapes.shape[0]
    dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
    tree = np.zeros((n, NODES_PER_CTU), TREE_DTYPE) if with_tree else None
    for c in range(n):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        rc = lib.fhevc_p_tree_select(shapes[c].ctypes.data, vw, vh, C.byref(rule), dmin[c].ctypes.data, dmax[c].ctypes.data, tree[c].ctypes.data if with_tree else None)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_tree_select")
    return (dmin, dmax, tree) if with_tree else (dmin, dmax)


def p_tree_select_merge(shapes, merge, width, height, rule=None, with_tree=False):
    """p_tree_select with the merge records [numCtus, 85] MOTION_MERGE_DTYPE beside the selection's: a node's own cost is the smaller of the two cost_best"""
    lib = load_library()
    rule = rule if rule is not None else p_tree_rule_default()
    shapes, merge = np.ascontiguousarray(shapes), np.ascontiguousarray(merge)
    assert shapes.dtype.itemsize == 16 and merge.dtype.itemsize == 16 and merge.shape == shapes.shape
    cw = (width + 63) // 64
    n = shapes.shape[0]
    dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
    tree = np.zeros((n, NODES_PER_CTU), TREE_DTYPE) if with_tree else None
    for c in range(n):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        rc = lib.fhevc_p_tree_select_merge(shapes[c].ctypes.data, merge[c].ctypes.data, vw, vh, C.byref(rule), dmin[c].ctypes.data, dmax[c].ctypes.data,
                                           tree[c].ctypes.data if with_tree else None)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_tree_select_merge")
    return (dmin, dmax, tree) if with_tree else (dmin, dmax)


def p_tree_select_skip(shapes, merge, skip, skip_mask, width, height, rule=None, with_tree=False):
    """p_tree_select_merge with the skip records [numCtus, 85] MOTION_SKIP_DTYPE: a node whose own cost is the merge cost and whose flags carry a bit of
    skip_mask (0..3) is not descended"""
    lib = load_library()
    rule = rule if rule is not None else p_tree_rule_default()
    shapes, merge, skip = np.ascontiguousarray(shapes), np.ascontiguousarray(merge), np.ascontiguousarray(skip)
    assert shapes.dtype.itemsize == 16 and merge.dtype.itemsize == 16 and skip.dtype.itemsize == 16 and merge.shape == shapes.shape == skip.shape
    cw = (width + 63) // 64
    n = shapes.shape[0]
    dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
    tree = np.zeros((n, NODES_PER_CTU), TREE_DTYPE) if with_tree else None
    for c in range(n):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        rc = lib.fhevc_p_tree_select_skip(shapes[c].ctypes.data, merge[c].ctypes.data, skip[c].ctypes.data, skip_mask, vw, vh, C.byref(rule), dmin[c].ctypes.data,
                                          dmax[c].ctypes.data, tree[c].ctypes.data if with_tree else None)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_tree_select_skip")
    return (dmin, dmax, tree) if with_tree else (dmin, dmax)


def p_tree_select_rd(rd_explicit, rd_merge, skip_mask, width, height, rule=None, with_tree=False):
    """p_tree_select_skip on RD records [numCtus, 85] MOTION_RD_DTYPE: rd_explicit's cost_rd stands for the selection's cost_best, rd_merge's cost_rd for the
    merge cost and rd_merge's flags for the skip flags"""
    lib = load_library()
    rule = rule if rule is not None else p_tree_rule_default()
    rd_explicit, rd_merge = np.ascontiguousarray(rd_explicit), np.ascontiguousarray(rd_merge)
    assert rd_explicit.dtype.itemsize == 16 and rd_merge.dtype.itemsize == 16 and rd_explicit.shape == rd_merge.shape
    cw = (width + 63) // 64
    n = rd_explicit.shape[0]
    dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
    tree = np.zeros((n, NODES_PER_CTU), TREE_DTYPE) if with_tree else None
    for c in range(n):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        rc = lib.fhevc_p_tree_select_rd(rd_explicit[c].ctypes.data, rd_merge[c].ctypes.data, skip_mask, vw, vh, C.byref(rule), dmin[c].ctypes.data,
                                        dmax[c].ctypes.data, tree[c].ctypes.data if with_tree else None)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_tree_select_rd")
    return (dmin, dmax, tree) if with_tree else (dmin, dmax)


def p_tree_select_rd_pu(rd_pu, rd_merge, skip_mask, width, height, rule=None, with_tree=False):
    """p_tree_select_rd with the folded records of motion_rd_pu [numCtus, 85] MOTION_RD_PU_DTYPE where rd_explicit stands; the same results"""
    rd_pu = np.ascontiguousarray(rd_pu)
    assert rd_pu.dtype == MOTION_RD_PU_DTYPE
    lib = load_library()
    rd_merge = np.ascontiguousarray(rd_merge)
    rule = rule if rule is not None else p_tree_rule_default()
    n, ctus_x = rd_pu.shape[0], (width + 63) // 64
    dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
    tree = np.zeros((n, NODES_PER_CTU), TREE_DTYPE)
    for c in range(n):
        vw, vh = min(64, width - (c % ctus_x) * 64), min(64, height - (c // ctus_x) * 64)
        rc = lib.fhevc_p_tree_select_rd_pu(rd_pu[c].ctypes.data, rd_merge[c].ctypes.data, skip_mask, vw, vh, C.byref(rule), dmin[c].ctypes.data,
                                           dmax[c].ctypes.data, tree[c].ctypes.data if with_tree else None)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_tree_select_rd_pu")
    return (dmin, dmax, tree) if with_tree else (dmin, dmax)


def p_tree_select_intra(shapes, merge, skip, skip_mask, intra, width, height, rule=None, with_tree=False):
    """p_tree_select_skip with the intra records [numCtus, 85] INTRA_P_DTYPE: a node that is not calm (merged with a masked zero bit) takes its intra cost
    where that is strictly smaller; bit TREE_INTRA of pad[0] of its tree record says so"""
    lib = load_library()
    rule = rule if rule is not None else p_tree_rule_default()
    shapes, merge, skip, intra = (np.ascontiguousarray(a) for a in (shapes, merge, skip, intra))
    assert all(a.dtype.itemsize == 16 and a.shape == shapes.shape for a in (shapes, merge, skip, intra))
    cw = (width + 63) // 64
    n = shapes.shape[0]
    dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
    tree = np.zeros((n, NODES_PER_CTU), TREE_DTYPE) if with_tree else None
    for c in range(n):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        rc = lib.fhevc_p_tree_select_intra(shapes[c].ctypes.data, merge[c].ctypes.data, skip[c].ctypes.data, skip_mask, intra[c].ctypes.data, vw, vh, C.byref(rule),
                                           dmin[c].ctypes.data, dmax[c].ctypes.data, tree[c].ctypes.data if with_tree else None)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_tree_select_intra")
    return (dmin, dmax, tree) if with_tree else (dmin, dmax)


def intra_p_picture(first, first4, width, height, qp=32, rows=None):
    """config 4, host side (no context, no device): the intra candidate costs of one picture's band from its first-pass records: first [band CTUs, 85],
    first4 [band CTUs, 256] or None (NODE_DTYPE; only satd and mode are read) -> [band CTUs, 85] INTRA_P_DTYPE"""
    lib = load_library()
    first = np.ascontiguousarray(first)
    first4 = None if first4 is None else np.ascontiguousarray(first4)
    rb, re = rows if rows is not None else (0, (height + 63) // 64)
    n = (re - rb) * ((width + 63) // 64)
    assert first.size == n * NODES_PER_CTU and first.dtype.itemsize == 16 and (first4 is None or (first4.size == n * PUS4_PER_CTU and first4.dtype.itemsize == 16))
    out = np.zeros((n, NODES_PER_CTU), INTRA_P_DTYPE)
    rc = lib.fhevc_intra_p_picture(width, height, rb, re, qp, first.ctypes.data, first4.ctypes.data if first4 is not None else None, out.ctypes.data)
    if rc != OK:
        raise FastHevcError(rc, "fhevc_intra_p_picture")
    return out


def pu_shape_select(nodes, pus, pus_small, width, height, rule=None, with_costs=False):
    """config 4, host side: the partition-size records [numCtus, 85] SHAPE_DTYPE of a P picture from its refined nodes [numCtus, 85], PUs [numCtus, 124]
    and small PUs [numCtus, 384] or None (MOTION_QPEL_DTYPE; only cost_best is read); with_costs: (records, costs [numCtus, 85, 8] uint32)"""
    lib = load_library()
    rule = rule if rule is not None else pu_shape_rule_default()
    nodes, pus = np.ascontiguousarray(nodes), np.ascontiguousarray(pus)
    small = None if pus_small is None else np.ascontiguousarray(pus_small)
    assert nodes.dtype.itemsize == 16 and pus.dtype.itemsize == 16 and (small is None or small.dtype.itemsize == 16)
    cw = (width + 63) // 64
    n = nodes.shape[0]
    out = np.zeros((n, NODES_PER_CTU), SHAPE_DTYPE)
    costs = np.zeros((n, NODES_PER_CTU, 8), np.uint32) if with_costs else None
    for c in range(n):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        rc = lib.fhevc_pu_shape_select(nodes[c].ctypes.data, pus[c].ctypes.data, None if small is None else small[c].ctypes.data, vw, vh, C.byref(rule),
                                       out[c].ctypes.data, costs[c].ctypes.data if with_costs else None)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_pu_shape_select")
    return (out, costs) if with_costs else out


def pu_shape_select_merge(nodes, pus, pus_small, merge_pus, merge_pus_small, width, height, rule=None, with_costs=False):
    """pu_shape_select with the PUs' merge records [numCtus, 124] and [numCtus, 384] or None (MOTION_MERGE_DTYPE; only cost_best is read) beside the refined
    entries: a part costs the smaller of the two -> (records, merged [numCtus, 85] uint16), with_costs: (records, costs, merged)"""
    lib = load_library()
    rule = rule if rule is not None else pu_shape_rule_default()
    cont = lambda a: None if a is None else np.ascontiguousarray(a)
    nodes, pus, small, mpus, msmall = cont(nodes), cont(pus), cont(pus_small), cont(merge_pus), cont(merge_pus_small)
    assert all(a is None or a.dtype.itemsize == 16 for a in (nodes, pus, small, mpus, msmall))
    at = lambda a, c: None if a is None else a[c].ctypes.data
    cw = (width + 63) // 64
    n = nodes.shape[0]
    out = np.zeros((n, NODES_PER_CTU), SHAPE_DTYPE)
    costs = np.zeros((n, NODES_PER_CTU, 8), np.uint32) if with_costs else None
    merged = np.zeros((n, NODES_PER_CTU), np.uint16)
    for c in range(n):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        rc = lib.fhevc_pu_shape_select_merge(nodes[c].ctypes.data, pus[c].ctypes.data, at(small, c), at(mpus, c), at(msmall, c), vw, vh, C.byref(rule),
                                             out[c].ctypes.data, at(costs, c), merged[c].ctypes.data)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_pu_shape_select_merge")
    return (out, costs, merged) if with_costs else (out, merged)


def _amvp_arrays(n_ctus, nodes, pus, pus_small, with_records, with_mvp):
    """the inputs of the re-pricing as contiguous [n_ctus, per] arrays (None stays None) and, per family that has an input, its zeroed outputs"""
    ins, outs, mvps = [], [], []
    for a, per in ((nodes, NODES_PER_CTU), (pus, PUS_PER_CTU), (pus_small, PUS_SMALL_PER_CTU)):
        if a is not None:
            a = np.ascontiguousarray(a).reshape(n_ctus, per)
            assert a.dtype.itemsize == 16
        ins.append(a)
        outs.append(np.zeros((n_ctus, per), MOTION_QPEL_DTYPE) if a is not None and with_records else None)
        mvps.append(np.zeros((n_ctus, per), MOTION_MVP_DTYPE) if a is not None and with_mvp else None)
    return ins, outs, mvps


def motion_amvp_picture(nodes, pus, pus_small, width, height, bit_depth=8, qp=32, rows=None, with_records=True, with_mvp=False):
    """config 4, host side (fhevc_motion_amvp_picture; no context, no device): the refined records [band CTUs, 85] / [.., 124] / [.., 384]
    (MOTION_QPEL_DTYPE; pus / pus_small may be None) re-priced against neighbour predictors -> (nodes, pus, pus_small) re-priced records, None for a
    family without input; with_mvp: behind them the three MOTION_MVP_DTYPE arrays; with_records=False: only those"""
    lib = load_library()
    cw, ch = (width + 63) // 64, (height + 63) // 64
    rb, re = rows if rows is not None else (0, ch)
    ins, outs, mvps = _amvp_arrays((re - rb) * cw, nodes, pus, pus_small, with_records, with_mvp)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = lib.fhevc_motion_amvp_picture(width, height, bit_depth, rb, re, qp, *[ptr(a) for a in ins + outs + mvps])
    if rc != OK:
        raise FastHevcError(rc, "fhevc_motion_amvp_picture")
    return tuple(outs if with_records else []) + tuple(mvps if with_mvp else [])


def p_depth_range(nodes, prev_depth, width, height, qp, rule=None):
    """config 4, host side: (depth_min, depth_max) [numCtus, 256] of a P picture from its motion nodes [numCtus, 85] and the
    co-located depths [numCtus, 256] of its reference picture"""
    lib = load_library()
    rule = rule if rule is not None else p_rule_default()
    nodes = np.ascontiguousarray(nodes)
    prev = np.ascontiguousarray(prev_depth, np.uint8)
    cw = (width + 63) // 64
    n = nodes.shape[0]
    dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
    for c in range(n):
        vw, vh = min(64, width - (c % cw) * 64), min(64, height - (c // cw) * 64)
        rc = lib.fhevc_p_depth_range(nodes[c].ctypes.data, prev[c].ctypes.data, vw, vh, qp, C.byref(rule), dmin[c].ctypes.data, dmax[c].ctypes.data)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_depth_range")
    return dmin, dmax


def p_motion_compensated_depth(nodes, prev_map, width, height):
    """config 4, host side: the reference picture's depths [numCtus, 256] seen through the motion nodes [numCtus, 85] of the current picture
    (the prev_depth argument of p_depth_range for content that moves)"""
    lib = load_library()
    nodes = np.ascontiguousarray(nodes)
    prev = np.ascontiguousarray(prev_map, np.uint8)
    out = np.zeros((nodes.shape[0], 256), np.uint8)
    for c in range(nodes.shape[0]):
        rc = lib.fhevc_p_motion_compensated_depth(nodes[c].ctypes.data, prev.ctypes.data, width, height, c, out[c].ctypes.data)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_motion_compensated_depth")
    return out


def p_node_depth(nodes, prev_map, width, height):
    """config 4, host side: the reference picture's depths seen through the motion, asked per CU node of the current picture's grid (a partition of
    every CTU: fhevc_p_node_depth)"""
    lib = load_library()
    nodes = np.ascontiguousarray(nodes)
    prev = np.ascontiguousarray(prev_map, np.uint8)
    out = np.zeros((nodes.shape[0], 256), np.uint8)
    for c in range(nodes.shape[0]):
        rc = lib.fhevc_p_node_depth(nodes[c].ctypes.data, prev.ctypes.data, width, height, c, out[c].ctypes.data)
        if rc != OK:
            raise FastHevcError(rc, "fhevc_p_node_depth")
    return out


def band(ctu_rows, rank, world):
    b, e = C.c_int(), C.c_int()
    rc = load_library().fhevc_band(ctu_rows, rank, world, C.byref(b), C.byref(e))
    if rc != OK:
        raise FastHevcError(rc, "fhevc_band")
    return b.value, e.value


class Context:
    """One fhevc_ctx: one picture geometry on one MI355X."""

    def __init__(self, width, height, bit_depth=8, weights=None, device=0, max_frames=1, arith=None, lib_path=None, devices=None):
        """devices: list of HIP ordinals for a multi-device context (the host-buffer entry points shard over them); default [device]"""
        self.lib = load_library(lib_path)
        self.width, self.height, self.bit_depth = width, height, bit_depth
        self.ctus_x, self.ctus_y = (width + 63) // 64, (height + 63) // 64
        self.num_ctus = self.ctus_x * self.ctus_y
        ids = list(devices) if devices else [device]
        dev = (C.c_int * len(ids))(*ids)
        cfg = Cfg(width, height, bit_depth, 64, 3, len(ids), dev, None, BACKEND_HIP, max_frames)
        h = C.c_void_p()
        rc = self.lib.fhevc_create(C.byref(h), C.byref(cfg))
        if rc != OK:
            raise FastHevcError(rc, "fhevc_create (no gfx950 device?)" if rc == E_NO_DEVICE else "fhevc_create")
        self.h = h
        if arith is not None:
            self.set_cnn_arith(arith)
        if weights is not None:
            self.set_weights(weights)

    def _check(self, rc):
        if rc != OK:
            raise FastHevcError(rc, self.lib.fhevc_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.fhevc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_weights(self, w):
        blob = w if isinstance(w, (bytes, bytearray)) else (_weights.pack_family(w) if "widths" in w else _weights.pack(w))
        self._check(self.lib.fhevc_set_weights(self.h, bytes(blob), len(blob)))

    def predict_frame(self, plane, origin=0, stride=None, qp=32, slice_type=2, want_hadamard=True):
        """plane: int16 numpy buffer holding a Pel plane; origin = element offset of sample (0,0)."""
        flat = np.ascontiguousarray(plane).reshape(-1)
        assert flat.dtype == np.int16
        stride = stride if stride is not None else plane.shape[-1]
        depth = np.zeros(self.num_ctus * 256, np.uint8)
        had = np.zeros(self.num_ctus, np.int32) if want_hadamard else None
        self._check(self.lib.fhevc_predict_frame(self.h, flat.ctypes.data + 2 * origin, stride, qp, slice_type,
                                                 depth.ctypes.data, had.ctypes.data if want_hadamard else None))
        return depth.reshape(self.num_ctus, 256), had

    def alloc_host(self, shape, dtype):
        """numpy array over pinned host memory of the library (fhevc_alloc_host); release with free_host(array)"""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = self.lib.fhevc_alloc_host(self.h, nbytes)
        if not p:
            raise FastHevcError(E_NOMEM, "fhevc_alloc_host")
        arr = np.frombuffer((C.c_uint8 * nbytes).from_address(p), dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def free_host(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            self.lib.fhevc_free_host(self.h, p)

    def predict_frames(self, luma, qp=32, want_hadamard=True, depth_out=None, had_out=None, origin=0, stride=None, frame_stride=None):
        """Host batch: luma [F, H, W] uint8 (8-bit content) or an int16 Pel buffer with origin/stride/frame_stride; returns
        (depth [F, numCtus, 256], hadamard [F, numCtus] or None) in host memory."""
        arr = np.asarray(luma)
        if arr.dtype == np.uint8:
            assert arr.ndim == 3 and arr.shape[1:] == (self.height, self.width) and arr.flags.c_contiguous
            nf, sb, st, fst, ptr = arr.shape[0], 1, self.width, self.width * self.height, arr.ctypes.data
        else:
            assert arr.dtype == np.int16 and arr.flags.c_contiguous and stride is not None and frame_stride is not None
            nf, sb, st, fst, ptr = arr.shape[0], 2, stride, frame_stride, arr.ctypes.data + 2 * origin
        depth = depth_out if depth_out is not None else np.zeros((nf, self.num_ctus, 256), np.uint8)
        had = had_out if had_out is not None else (np.zeros((nf, self.num_ctus), np.int32) if want_hadamard else None)
        self._check(self.lib.fhevc_predict_frames(self.h, ptr, sb, st, fst, nf, qp, depth.ctypes.data, had.ctypes.data if had is not None else None))
        return depth, had

    def predict_frame_range(self, plane, origin=0, stride=None, qp=32, margin=0, slice_type=2, margin_stop=None, with_hadamard=False):
        """Soft decisions: (depth_min, depth_max), each [numCtus, 256] (and the per-CTU source Hadamard when asked for)."""
        flat = np.ascontiguousarray(plane).reshape(-1)
        assert flat.dtype == np.int16
        stride = stride if stride is not None else plane.shape[-1]
        dmin = np.zeros(self.num_ctus * 256, np.uint8)
        dmax = np.zeros(self.num_ctus * 256, np.uint8)
        had = np.zeros(self.num_ctus, np.int32) if with_hadamard else None
        self._check(self.lib.fhevc_predict_frame_range(self.h, flat.ctypes.data + 2 * origin, stride, qp, slice_type, margin,
                                                       margin if margin_stop is None else margin_stop,
                                                       dmin.ctypes.data, dmax.ctypes.data, had.ctypes.data if with_hadamard else None))
        out = (dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256))
        return out + (had,) if with_hadamard else out

    def satd(self, org, cur, w, h, bit_depth=8, org_stride=None, cur_stride=None):
        org = np.ascontiguousarray(org, np.int16)
        cur = np.ascontiguousarray(cur, np.int16)
        out = C.c_uint32()
        self._check(self.lib.fhevc_satd(self.h, org.ctypes.data, org_stride or org.shape[-1], cur.ctypes.data,
                                        cur_stride or cur.shape[-1], w, h, bit_depth, C.byref(out)))
        return out.value

    def intra_first_pass(self, plane, origin=0, stride=None, qp=32):
        flat = np.ascontiguousarray(plane).reshape(-1)
        stride = stride if stride is not None else plane.shape[-1]
        out = np.zeros(self.num_ctus * NODES_PER_CTU, NODE_DTYPE)
        self._check(self.lib.fhevc_intra_first_pass(self.h, flat.ctypes.data + 2 * origin, stride, qp, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def _pair(self, cur_plane, ref_plane, origin, stride):
        """the picture pair of a host form -> (pointer to sample (0, 0) of cur, of ref, stride in samples); each pointer keeps its (contiguous) array alive"""
        out = []
        for plane in (cur_plane, ref_plane):
            flat = np.ascontiguousarray(plane).reshape(-1)
            assert flat.dtype == np.int16
            p = C.c_void_p(flat.ctypes.data + 2 * origin)
            p._array = flat
            out.append(p)
        return out[0], out[1], stride if stride is not None else cur_plane.shape[-1]

    _FAMILIES = (NODES_PER_CTU, PUS_PER_CTU, PUS_SMALL_PER_CTU)

    def _search_families(self, *wanted):
        """(nodes, pus, pus_small) flags -> (outputs of MOTION_DTYPE, None for a family not asked for; their pointers)"""
        outs = [np.zeros(self.num_ctus * per_ctu, MOTION_DTYPE) if want else None for want, per_ctu in zip(wanted, self._FAMILIES)]
        return outs, [None if o is None else o.ctypes.data for o in outs]

    def _refine_families(self, *arrays, dtype=None):
        """(nodes, pus, pus_small) arrays of 16-byte entries (of `dtype`, where given), None for a family left out -> (flat inputs, outputs of
        MOTION_QPEL_DTYPE, the pointers in, out per family)"""
        ins, outs, ptrs = [], [], []
        for a, per_ctu in zip(arrays, self._FAMILIES):
            if a is not None:
                a = np.ascontiguousarray(a).reshape(-1)
                assert (a.dtype.itemsize == 16 if dtype is None else a.dtype == dtype) and a.size == self.num_ctus * per_ctu
            ins.append(a)
            outs.append(None if a is None else np.zeros(a.size, MOTION_QPEL_DTYPE))
            ptrs += [None if a is None else a.ctypes.data, None if a is None else outs[-1].ctypes.data]
        return ins, outs, ptrs

    def _per_ctu(self, outs):
        return tuple(None if o is None else o.reshape(self.num_ctus, -1) for o in outs)

    def motion_search(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=4):
        """config 4: [numCtus, 85] MOTION_DTYPE nodes of cur searched in ref (two Pel planes of the same layout)."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_DTYPE)
        self._check(self.lib.fhevc_motion_search(self.h, cur, ref, stride, qp,
                                                 search_range, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def motion_search_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_out, rows=None, stream=None, qp=32,
                             search_range=4):
        """frames 1.. of the batch, each searched in the frame before it; d_out: (num_frames - 1) * band CTUs * 85 nodes (16 B)."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_search_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp,
                                                        search_range, d_out, stream))

    def motion_refine(self, cur_plane, ref_plane, nodes, origin=0, stride=None, qp=32, max_range=4):
        """config 4: the quarter-sample refinement of nodes [numCtus, 85] (MOTION_DTYPE, as motion_search returns them for the same planes; only
        mvx / mvy are read) -> [numCtus, 85] MOTION_QPEL_DTYPE.  max_range: the search's range (a longer vector gets the marker)."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        nodes = np.ascontiguousarray(nodes).reshape(-1)
        assert nodes.dtype.itemsize == 16 and nodes.size == self.num_ctus * NODES_PER_CTU
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_QPEL_DTYPE)
        self._check(self.lib.fhevc_motion_refine(self.h, cur, ref, stride, qp, max_range,
                                                 nodes.ctypes.data, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def motion_refine_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_nodes, d_out, rows=None, stream=None, qp=32,
                             max_range=4):
        """frames 1.. of the batch, each refined in the frame before it, around the vectors of d_nodes (what motion_search_device wrote for the same
        rows); d_out: (num_frames - 1) * band CTUs * 85 quarter-sample nodes (16 B).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_refine_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range,
                                                        d_nodes, d_out, stream))

    def motion_merge(self, cur_plane, ref_plane, refined, origin=0, stride=None, qp=32, max_range=4):
        """config 4: the cheapest merge candidate of every CU node from the refined nodes [numCtus, 85] (MOTION_QPEL_DTYPE, as motion_refine returns them
        for the same planes; only cost_best, mvx, mvy are read) -> [numCtus, 85] MOTION_MERGE_DTYPE.  max_range: the refinement's."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        refined = np.ascontiguousarray(refined).reshape(-1)
        assert refined.dtype.itemsize == 16 and refined.size == self.num_ctus * NODES_PER_CTU
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_MERGE_DTYPE)
        self._check(self.lib.fhevc_motion_merge(self.h, cur, ref, stride, qp, max_range,
                                                refined.ctypes.data, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def motion_merge_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_refined, d_out, rows=None, stream=None, qp=32, max_range=4):
        """frames 1.. of the batch, each predicted from the frame before it, at the vectors of the neighbours' records in d_refined (what a refinement wrote
        for the same rows: 85 per CTU); d_out: (num_frames - 1) * band CTUs * 85 merge records (16 B).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_merge_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range,
                                                       d_refined, d_out, stream))

    def motion_skip(self, cur_plane, ref_plane, merge, origin=0, stride=None, qp=32, max_range=4):
        """config 4: the zero-residual test of every CU node at the vector of its merge record [numCtus, 85] (MOTION_MERGE_DTYPE, as motion_merge returns
        them for the same planes; only cost_best, mvx, mvy are read) -> [numCtus, 85] MOTION_SKIP_DTYPE.  max_range: the merge stage's."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        merge = np.ascontiguousarray(merge).reshape(-1)
        assert merge.dtype.itemsize == 16 and merge.size == self.num_ctus * NODES_PER_CTU
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_SKIP_DTYPE)
        self._check(self.lib.fhevc_motion_skip(self.h, cur, ref, stride, qp, max_range, merge.ctypes.data, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def motion_skip_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_merge, d_out, rows=None, stream=None, qp=32, max_range=4):
        """frames 1.. of the batch, each predicted from the frame before it at the vectors of d_merge (what motion_merge_device wrote for the same rows:
        85 per CTU), transformed and quantised at qp; d_out: (num_frames - 1) * band CTUs * 85 skip records (16 B).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_skip_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range,
                                                      d_merge, d_out, stream))

    def motion_rd(self, cur_plane, ref_plane, records, source, mvp=None, origin=0, stride=None, qp=32, max_range=4):
        """config 4: the RD estimate of every CU node at the vector of its record [numCtus, 85] -- source RD_SOURCE_MERGE: MOTION_MERGE_DTYPE, RD_SOURCE_EXPLICIT:
        MOTION_QPEL_DTYPE, with the re-pricing's predictor records mvp [numCtus, 85] MOTION_MVP_DTYPE or None -> [numCtus, 85] MOTION_RD_DTYPE"""
        return self.motion_rd_qt(cur_plane, ref_plane, records, source, None, mvp, origin, stride, qp, max_range)

    def motion_rd_qt(self, cur_plane, ref_plane, records, source, tu_depths=3, mvp=None, origin=0, stride=None, qp=32, max_range=4):
        """motion_rd at tu_depths TU depths: 2 -- motion_rd's bytes, 3 -- HM's full residual quad-tree (the 32x32 and 16x16 nodes get their third TU size;
        tu_split bits 4..7).  None: the entry point without the argument"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        records = np.ascontiguousarray(records).reshape(-1)
        assert records.dtype.itemsize == 16 and records.size == self.num_ctus * NODES_PER_CTU
        if mvp is not None:
            mvp = np.ascontiguousarray(mvp).reshape(-1)
            assert mvp.dtype.itemsize == 8 and mvp.size == records.size
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_RD_DTYPE)
        head = (self.h, cur, ref, stride, qp, max_range, source, records.ctypes.data, mvp.ctypes.data if mvp is not None else None)
        self._check(self.lib.fhevc_motion_rd(*head, out.ctypes.data) if tu_depths is None else self.lib.fhevc_motion_rd_qt(*head, tu_depths, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def motion_rd_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, source, d_in, d_out, d_mvp=None, rows=None, stream=None, qp=32, max_range=4):
        """frames 1.. of the batch, each predicted from the frame before it at the vectors of d_in (85 records of `source`'s kind per CTU, compact over the
        rows; d_mvp: their predictor records or None), transformed, quantised and rebuilt at qp; d_out: (num_frames - 1) * band CTUs * 85 RD records (16 B).
        Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_rd_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range, source,
                                                    d_in, d_mvp, d_out, stream))

    def motion_rd_qt_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, source, d_in, tu_depths, d_out, d_mvp=None, rows=None, stream=None, qp=32,
                            max_range=4):
        """motion_rd_device at tu_depths (2 or 3) TU depths.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_rd_qt_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range, source,
                                                       d_in, d_mvp, tu_depths, d_out, stream))

    @staticmethod
    def rd_pu_inputs(nodes, pus=None, pus_small=None, merge_pus=None, merge_pus_small=None, mvp_nodes=None, mvp_pus=None, mvp_pus_small=None, shapes=None, fold=None):
        """fhevc_motion_rd_pu_inputs from device addresses (integers), None for an array left out"""
        return MotionRdPuInputs(nodes, pus, pus_small, merge_pus, merge_pus_small, mvp_nodes, mvp_pus, mvp_pus_small, shapes, fold)

    def motion_rd_pu(self, cur_plane, ref_plane, part_mode, nodes, pus=None, pus_small=None, merge_pus=None, merge_pus_small=None, mvp_nodes=None, mvp_pus=None,
                     mvp_pus_small=None, shapes=None, fold=None, origin=0, stride=None, qp=32, max_range=4):
        """config 4: the RD estimate of every CU node under a partition size -- part_mode a PART_* number, RD_PART_BEST or RD_PART_SECOND (of shapes) -- with the
        prediction composed from the two parts' vectors: nodes / pus / pus_small [numCtus, 85 / 124 / 384] MOTION_QPEL_DTYPE, their merge records
        (MOTION_MERGE_DTYPE) and predictor records (MOTION_MVP_DTYPE) or None, shapes [numCtus, 85] SHAPE_DTYPE, fold: an earlier call's result to fold into
        -> [numCtus, 85] MOTION_RD_PU_DTYPE"""
        return self.motion_rd_pu_qt(cur_plane, ref_plane, part_mode, nodes, None, pus, pus_small, merge_pus, merge_pus_small, mvp_nodes, mvp_pus, mvp_pus_small, shapes,
                                    fold, origin, stride, qp, max_range)

    def motion_rd_pu_qt(self, cur_plane, ref_plane, part_mode, nodes, tu_depths=3, pus=None, pus_small=None, merge_pus=None, merge_pus_small=None, mvp_nodes=None,
                        mvp_pus=None, mvp_pus_small=None, shapes=None, fold=None, origin=0, stride=None, qp=32, max_range=4):
        """motion_rd_pu at tu_depths TU depths (2: motion_rd_pu's bytes; 3: HM's full residual quad-tree; None: the entry point without the argument); fold may
        come from a call at either depth count"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        keep, ptrs = [], []
        for a, per_ctu, size in ((nodes, 85, 16), (pus, 124, 16), (pus_small, 384, 16), (merge_pus, 124, 16), (merge_pus_small, 384, 16), (mvp_nodes, 85, 8),
                                 (mvp_pus, 124, 8), (mvp_pus_small, 384, 8), (shapes, 85, 16), (fold, 85, 16)):
            if a is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(a).reshape(-1)
            assert a.dtype.itemsize == size and a.size == self.num_ctus * per_ctu
            keep.append(a)
            ptrs.append(a.ctypes.data)
        inputs = MotionRdPuInputs(*ptrs)
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_RD_PU_DTYPE)
        head = (self.h, cur, ref, stride, qp, max_range, part_mode, C.byref(inputs))
        self._check(self.lib.fhevc_motion_rd_pu(*head, out.ctypes.data) if tu_depths is None else self.lib.fhevc_motion_rd_pu_qt(*head, tu_depths, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def motion_rd_pu_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, part_mode, inputs, d_out, rows=None, stream=None, qp=32, max_range=4):
        """frames 1.. of the batch, each predicted from the frame before it with every node's prediction composed from the two parts of its partition size
        (inputs: rd_pu_inputs(...) of device addresses, compact over the rows); d_out: (num_frames - 1) * band CTUs * 85 records (16 B), folded into
        inputs.fold where that is given (d_out itself is allowed).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_rd_pu_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range, part_mode,
                                                       C.byref(inputs) if inputs is not None else None, d_out, stream))

    def motion_rd_pu_qt_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, part_mode, inputs, tu_depths, d_out, rows=None, stream=None, qp=32,
                               max_range=4):
        """motion_rd_pu_device at tu_depths (2 or 3) TU depths; inputs.fold may hold records of either depth count.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_rd_pu_qt_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range, part_mode,
                                                          C.byref(inputs) if inputs is not None else None, tu_depths, d_out, stream))

    def intra_rd(self, plane, first, fold=None, rd_merge=None, skip_mask=0, origin=0, stride=None, qp=32):
        """config 4: the RD estimate of the intra candidate of every CU node of one picture -- first [numCtus, 85] NODE_DTYPE (the first pass's records: the
        mode priced), fold: MOTION_RD_PU_DTYPE records to fold into or None, rd_merge: MOTION_RD_DTYPE records for the calm gate under skip_mask or None
        -> [numCtus, 85] MOTION_RD_PU_DTYPE (part RD_PART_INTRA, the mode in pad[0], where the intra candidate was written)"""
        return self.intra_rd_qt(plane, first, None, fold, rd_merge, skip_mask, origin, stride, qp)

    def intra_rd_qt(self, plane, first, tu_depths=3, fold=None, rd_merge=None, skip_mask=0, origin=0, stride=None, qp=32):
        """intra_rd with the number of TU depths: 2 -- intra_rd's bytes; 3 -- HM's full intra TU tree: 32x32 nodes get 8x8 TUs, 16x16 and 8x8 nodes 4x4 TUs
        on the DST, tu_split bits 4..7 say which depth-1 TU split (None: the entry point without the argument)"""
        flat = np.ascontiguousarray(plane).reshape(-1)
        assert flat.dtype == np.int16
        stride = stride if stride is not None else plane.shape[-1]
        arrays = []
        for a in (first, fold, rd_merge):
            if a is not None:
                a = np.ascontiguousarray(a).reshape(-1)
                assert a.dtype.itemsize == 16 and a.size == self.num_ctus * NODES_PER_CTU
            arrays.append(a)
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_RD_PU_DTYPE)
        head = (self.h, flat.ctypes.data + 2 * origin, stride, qp, *[a.ctypes.data if a is not None else None for a in arrays], skip_mask)
        self._check(self.lib.fhevc_intra_rd(*head, out.ctypes.data) if tu_depths is None else self.lib.fhevc_intra_rd_qt(*head, tu_depths, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def intra_rd_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_first, d_out, d_fold=None, d_rd_merge=None, skip_mask=0, rows=None, stream=None,
                        qp=32):
        """every picture of the batch (no pairing): d_first num_frames * band CTUs * 85 first-pass records, d_out as many RD records (16 B), gated by d_rd_merge
        under skip_mask and folded into d_fold where those are given (d_fold may be d_out).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_intra_rd_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, d_first, d_fold, d_rd_merge, skip_mask,
                                                   d_out, stream))

    def intra_rd_qt_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_first, tu_depths, d_out, d_fold=None, d_rd_merge=None, skip_mask=0, rows=None,
                           stream=None, qp=32):
        """intra_rd_device with the number of TU depths (2 or 3) in front of the output.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_intra_rd_qt_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, d_first, d_fold, d_rd_merge, skip_mask,
                                                      tu_depths, d_out, stream))

    def intra_rd_nxn(self, plane, first, first4=None, fold=None, rd_merge=None, skip_mask=0, origin=0, stride=None, qp=32, with_nxn=False):
        """intra_rd_qt at 3 with the NxN candidate of the 8x8 nodes: first4 [numCtus, 256] NODE_DTYPE (the 4x4 first pass's records: the four modes priced;
        None: intra_rd_qt's bytes at 3) -> [numCtus, 85] MOTION_RD_PU_DTYPE (part RD_PART_INTRA_NXN where NxN was taken); with_nxn: and the plain candidates
        [numCtus, 64] INTRA_RD_NXN_DTYPE"""
        flat = np.ascontiguousarray(plane).reshape(-1)
        assert flat.dtype == np.int16
        stride = stride if stride is not None else plane.shape[-1]
        arrays = []
        for a, per_ctu in ((first, NODES_PER_CTU), (first4, 256), (fold, NODES_PER_CTU), (rd_merge, NODES_PER_CTU)):
            if a is not None:
                a = np.ascontiguousarray(a).reshape(-1)
                assert a.dtype.itemsize == 16 and a.size == self.num_ctus * per_ctu
            arrays.append(a)
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_RD_PU_DTYPE)
        nxn = np.zeros(self.num_ctus * NXN_PER_CTU, INTRA_RD_NXN_DTYPE) if with_nxn else None
        self._check(self.lib.fhevc_intra_rd_nxn(self.h, flat.ctypes.data + 2 * origin, stride, qp, *[a.ctypes.data if a is not None else None for a in arrays], skip_mask,
                                                out.ctypes.data, nxn.ctypes.data if with_nxn else None))
        out = out.reshape(self.num_ctus, NODES_PER_CTU)
        return (out, nxn.reshape(self.num_ctus, NXN_PER_CTU)) if with_nxn else out

    def intra_rd_nxn_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_first, d_first4, d_out, d_nxn=None, d_fold=None, d_rd_merge=None, skip_mask=0,
                            rows=None, stream=None, qp=32):
        """intra_rd_qt_device at 3 with the NxN candidate: d_first4 num_frames * band CTUs * 256 records of the 4x4 first pass (None: that call's bytes and
        launch), d_nxn: as many CTUs * 64 NxN records (16 B) or None.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_intra_rd_nxn_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, d_first, d_first4, d_fold, d_rd_merge,
                                                       skip_mask, d_out, d_nxn, stream))

    def intra_rd_search(self, plane, modes, modes4=None, rule=None, fold=None, rd_merge=None, skip_mask=0, origin=0, stride=None, qp=32, with_nxn=False):
        """intra_rd_nxn with the mode searched over the first pass's lists: modes [numCtus, 85, list_stride] uint8, modes4 [numCtus, 256, list_stride4] uint8 (None:
        no NxN candidate); rule: an IntraSearchRule (None: the default) -> [numCtus, 85] MOTION_RD_PU_DTYPE (pad[1]: the winner's list position); with_nxn: and the
        plain NxN candidates [numCtus, 64] INTRA_RD_NXN_DTYPE"""
        flat = np.ascontiguousarray(plane).reshape(-1)
        assert flat.dtype == np.int16
        stride = stride if stride is not None else plane.shape[-1]
        modes = np.ascontiguousarray(modes, np.uint8).reshape(self.num_ctus, NODES_PER_CTU, -1)
        if modes4 is not None:
            modes4 = np.ascontiguousarray(modes4, np.uint8).reshape(self.num_ctus, 256, -1)
        arrays = []
        for a in (fold, rd_merge):
            if a is not None:
                a = np.ascontiguousarray(a).reshape(-1)
                assert a.dtype.itemsize == 16 and a.size == self.num_ctus * NODES_PER_CTU
            arrays.append(a)
        rule = rule if rule is not None else intra_search_rule_default()
        out = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_RD_PU_DTYPE)
        nxn = np.zeros(self.num_ctus * NXN_PER_CTU, INTRA_RD_NXN_DTYPE) if with_nxn else None
        self._check(self.lib.fhevc_intra_rd_search(self.h, flat.ctypes.data + 2 * origin, stride, qp, modes.ctypes.data, modes.shape[2],
                                                   modes4.ctypes.data if modes4 is not None else None, modes4.shape[2] if modes4 is not None else 0, C.byref(rule),
                                                   *[a.ctypes.data if a is not None else None for a in arrays], skip_mask, out.ctypes.data,
                                                   nxn.ctypes.data if with_nxn else None))
        out = out.reshape(self.num_ctus, NODES_PER_CTU)
        return (out, nxn.reshape(self.num_ctus, NXN_PER_CTU)) if with_nxn else out

    def intra_rd_search_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_modes, list_stride, d_modes4, list_stride4, d_out, rule=None, d_nxn=None,
                               d_fold=None, d_rd_merge=None, skip_mask=0, rows=None, stream=None, qp=32):
        """intra_rd_nxn_device with the mode searched over the lists: d_modes num_frames * band CTUs * 85 * list_stride bytes, d_modes4 as many CTUs * 256 *
        list_stride4 bytes or None; rule: an IntraSearchRule (None: the default), read before the call returns.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        rule = rule if rule is not None else intra_search_rule_default()
        self._check(self.lib.fhevc_intra_rd_search_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, d_modes, list_stride, d_modes4,
                                                          list_stride4, C.byref(rule), d_fold, d_rd_merge, skip_mask, d_out, d_nxn, stream))

    def motion_merge_pu(self, cur_plane, ref_plane, refined, origin=0, stride=None, qp=32, max_range=4, with_pus=True, with_small=True):
        """config 4: the cheapest merge candidate of every PU from the refined square nodes [numCtus, 85] (MOTION_QPEL_DTYPE; only cost_best, mvx, mvy are
        read) -> ([numCtus, 124], [numCtus, 384]) MOTION_MERGE_DTYPE in the orders of motion_pu_index / motion_pu_small_index; None for a family not asked for"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        refined = np.ascontiguousarray(refined).reshape(-1)
        assert refined.dtype.itemsize == 16 and refined.size == self.num_ctus * NODES_PER_CTU
        pus = np.zeros((self.num_ctus, PUS_PER_CTU), MOTION_MERGE_DTYPE) if with_pus else None
        small = np.zeros((self.num_ctus, PUS_SMALL_PER_CTU), MOTION_MERGE_DTYPE) if with_small else None
        self._check(self.lib.fhevc_motion_merge_pu(self.h, cur, ref, stride, qp, max_range, refined.ctypes.data, pus.ctypes.data if with_pus else None,
                                                   small.ctypes.data if with_small else None))
        return pus, small

    def motion_merge_pu_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_refined, d_out_pus, d_out_pus_small, rows=None, stream=None, qp=32,
                               max_range=4):
        """motion_merge_device per PU: d_refined as there (85 refined nodes per CTU); d_out_pus: (num_frames - 1) * band CTUs * 124 merge records,
        d_out_pus_small: ... * 384; either may be None, not both.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_merge_pu_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range,
                                                          d_refined, d_out_pus, d_out_pus_small, stream))

    def motion_amvp(self, nodes, pus=None, pus_small=None, qp=32, with_records=True, with_mvp=False):
        """config 4: the refined records of one picture [numCtus, 85] / [numCtus, 124] / [numCtus, 384] (MOTION_QPEL_DTYPE; pus / pus_small may be None)
        re-priced against neighbour predictors on the device -> as motion_amvp_picture"""
        ins, outs, mvps = _amvp_arrays(self.num_ctus, nodes, pus, pus_small, with_records, with_mvp)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._check(self.lib.fhevc_motion_amvp(self.h, qp, *[ptr(a) for a in ins + outs + mvps]))
        return tuple(outs if with_records else []) + tuple(mvps if with_mvp else [])

    def motion_amvp_device(self, num_frames, d_nodes, d_pus=None, d_pus_small=None, d_out_nodes=None, d_out_pus=None, d_out_pus_small=None, d_mvp_nodes=None,
                           d_mvp_pus=None, d_mvp_pus_small=None, rows=None, stream=None, qp=32):
        """the refined records of num_frames - 1 picture pairs (85 / 124 / 384 per CTU, compact over the rows) re-priced against neighbour predictors;
        d_out_*: as many records (16 B), d_mvp_*: as many predictor records (8 B); each output may be None, not all six.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_amvp_device(self.h, num_frames, rb, re, qp, d_nodes, d_pus, d_pus_small, d_out_nodes, d_out_pus, d_out_pus_small,
                                                      d_mvp_nodes, d_mvp_pus, d_mvp_pus_small, stream))

    def motion_search_pu(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=4, with_nodes=False):
        """config 4: the search of motion_search for the rectangular PUs -> [numCtus, 124] MOTION_DTYPE in the order of motion_pu_index; with_nodes:
        (nodes [numCtus, 85], pus), the nodes as motion_search returns them, from the same pass.  search_range 1..8."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        pus = np.zeros(self.num_ctus * PUS_PER_CTU, MOTION_DTYPE)
        nodes = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_DTYPE) if with_nodes else None
        self._check(self.lib.fhevc_motion_search_pu(self.h, cur, ref, stride, qp, search_range,
                                                    nodes.ctypes.data if with_nodes else None, pus.ctypes.data))
        pus = pus.reshape(self.num_ctus, PUS_PER_CTU)
        return (nodes.reshape(self.num_ctus, NODES_PER_CTU), pus) if with_nodes else pus

    def motion_search_pu_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_pus, d_nodes=None, rows=None, stream=None, qp=32,
                                search_range=4):
        """frames 1.. of the batch, each searched in the frame before it; d_pus: (num_frames - 1) * band CTUs * 124 entries (16 B); d_nodes (optional):
        (num_frames - 1) * band CTUs * 85, what motion_search_device writes for the same arguments.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_search_pu_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, search_range,
                                                           d_nodes, d_pus, stream))

    def motion_search_pu_small(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=4):
        """config 4: the search of motion_search for the PUs with a 4-sample side (AMP of 16x16 CUs, 8x4 / 4x8) -> [numCtus, 384] MOTION_DTYPE in the order
        of motion_pu_small_index.  search_range 1..8."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        pus = np.zeros(self.num_ctus * PUS_SMALL_PER_CTU, MOTION_DTYPE)
        self._check(self.lib.fhevc_motion_search_pu_small(self.h, cur, ref, stride, qp, search_range,
                                                          pus.ctypes.data))
        return pus.reshape(self.num_ctus, PUS_SMALL_PER_CTU)

    def motion_search_pu_small_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_pus, rows=None, stream=None, qp=32, search_range=4):
        """frames 1.. of the batch, each searched in the frame before it; d_pus: (num_frames - 1) * band CTUs * 384 entries (16 B).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_search_pu_small_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, search_range,
                                                                 d_pus, stream))

    def motion_search_pu_wide(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=64, nodes=True, pus=True, pus_small=True):
        """config 4: the SAD search of motion_search, motion_search_pu and motion_search_pu_small at search_range 1..64 from one call ->
        (nodes [numCtus, 85], pus [numCtus, 124], pus_small [numCtus, 384]) of MOTION_DTYPE, None for a family not asked for (at least one must be)."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        outs, p = self._search_families(nodes, pus, pus_small)
        self._check(self.lib.fhevc_motion_search_pu_wide(self.h, cur, ref, stride, qp, search_range, *p))
        return self._per_ctu(outs)

    def motion_search_pu_wide_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_nodes=None, d_pus=None, d_pus_small=None, rows=None,
                                     stream=None, qp=32, search_range=64):
        """frames 1.. of the batch, each searched in the frame before it, SAD, search_range 1..64; d_nodes / d_pus / d_pus_small: (num_frames - 1) * band
        CTUs * 85 / 124 / 384 entries (16 B), each optional (not all three).  Asynchronous; keeps no state between calls."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_search_pu_wide_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, search_range,
                                                                d_nodes, d_pus, d_pus_small, stream))

    def motion_centres(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, coarse_range=14):
        """config 4: one coarse motion centre per CTU from the 4:1 decimated pair (coarse_range 1..14 cells) -> [numCtus] of MOTION_DTYPE; mvx / mvy are
        multiples of 4 within +-56 whole samples.  This library's own definition (include/fasthevc.h), no HM counterpart."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        out = np.zeros(self.num_ctus, MOTION_DTYPE)
        self._check(self.lib.fhevc_motion_centres(self.h, cur, ref, stride, qp, coarse_range, out.ctypes.data))
        return out

    def motion_centres_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_centres, rows=None, stream=None, qp=32, coarse_range=14):
        """frames 1.. of the batch, each searched in the frame before it; d_centres: (num_frames - 1) * band CTUs entries (16 B), one per CTU.
        Asynchronous; keeps no state between calls."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_centres_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, coarse_range,
                                                         d_centres, stream))

    def motion_search_pu_centred(self, cur_plane, ref_plane, centres, origin=0, stride=None, qp=32, search_range=8, nodes=True, pus=True, pus_small=True):
        """config 4: the SAD searches of motion_search_pu_wide in a window of +-search_range (1..8) around one centre per CTU (centres: [numCtus] of
        MOTION_DTYPE, as motion_centres returns them; only mvx / mvy are read) -> (nodes, pus, pus_small) with ABSOLUTE vectors, None for a family not asked for."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        cen = np.ascontiguousarray(centres).reshape(-1)
        assert cen.dtype == MOTION_DTYPE and cen.size == self.num_ctus
        outs, p = self._search_families(nodes, pus, pus_small)
        self._check(self.lib.fhevc_motion_search_pu_centred(self.h, cur, ref, stride, qp, search_range, cen.ctypes.data, *p))
        return self._per_ctu(outs)

    def motion_search_pu_centred_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_centres, d_nodes=None, d_pus=None, d_pus_small=None,
                                        rows=None, stream=None, qp=32, search_range=8):
        """frames 1.. of the batch, each searched in the frame before it around d_centres ((num_frames - 1) * band CTUs entries, as motion_centres_device
        writes them); outputs as motion_search_pu_wide_device.  Asynchronous; keeps no state between calls."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_search_pu_centred_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, search_range,
                                                                   d_centres, d_nodes, d_pus, d_pus_small, stream))

    def motion_refine_pu_centred(self, cur_plane, ref_plane, centres, origin=0, stride=None, qp=32, max_range=8, nodes=None, pus=None, pus_small=None):
        """config 4: the quarter-sample refinement of motion_search_pu_centred's vectors, priced against the CTU's centre: nodes [numCtus, 85], pus
        [numCtus, 124], pus_small [numCtus, 384] (MOTION_DTYPE, absolute vectors; only mvx / mvy are read), centres [numCtus] -> (out_nodes, out_pus,
        out_pus_small) of MOTION_QPEL_DTYPE, None for a family not given.  max_range 1..8 around the centre."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        cen = np.ascontiguousarray(centres).reshape(-1)
        assert cen.dtype == MOTION_DTYPE and cen.size == self.num_ctus
        ins, outs, p = self._refine_families(nodes, pus, pus_small, dtype=MOTION_DTYPE)
        self._check(self.lib.fhevc_motion_refine_pu_centred(self.h, cur, ref, stride, qp, max_range, cen.ctypes.data, *p))
        return self._per_ctu(outs)

    def motion_refine_pu_centred_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_centres, d_nodes=None, d_out_nodes=None, d_pus=None,
                                        d_out_pus=None, d_pus_small=None, d_out_pus_small=None, rows=None, stream=None, qp=32, max_range=8):
        """frames 1.. of the batch, each refined in the frame before it around d_centres; inputs as motion_search_pu_centred_device wrote them for the same
        rows, outputs as many quarter-sample entries (16 B).  Each in / out pair is optional (not all three).  Asynchronous; keeps no state between calls."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_refine_pu_centred_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range, d_centres,
                                                                   d_nodes, d_out_nodes, d_pus, d_out_pus, d_pus_small, d_out_pus_small, stream))

    def motion_refine_pu(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, max_range=4, pus=None, pus_small=None):
        """config 4: the quarter-sample refinement of the PUs' vectors: pus [numCtus, 124] and / or pus_small [numCtus, 384] (MOTION_DTYPE, as
        motion_search_pu / motion_search_pu_small return them for the same planes; only mvx / mvy are read) -> (out_pus, out_pus_small) of
        MOTION_QPEL_DTYPE in the same layouts, None for a family not given.  max_range 1..8: the search's range (a longer vector gets the marker)."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        ins, outs, p = self._refine_families(None, pus, pus_small)
        self._check(self.lib.fhevc_motion_refine_pu(self.h, cur, ref, stride, qp, max_range, *p[2:]))
        return self._per_ctu(outs[1:])

    def motion_refine_pu_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_pus, d_out_pus, d_pus_small, d_out_pus_small, rows=None,
                                stream=None, qp=32, max_range=4):
        """frames 1.. of the batch, each refined in the frame before it, around the vectors of d_pus (what motion_search_pu_device wrote for the same
        rows; 124 per CTU) and d_pus_small (motion_search_pu_small_device; 384 per CTU); the outputs hold as many quarter-sample entries (16 B).
        Either family's pair may be None together.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_refine_pu_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range,
                                                           d_pus, d_out_pus, d_pus_small, d_out_pus_small, stream))

    def motion_refine_pu_wide(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, max_range=64, nodes=None, pus=None, pus_small=None):
        """config 4: the quarter-sample refinements of motion_refine and motion_refine_pu at max_range 1..64 from one call: nodes [numCtus, 85], pus
        [numCtus, 124] and / or pus_small [numCtus, 384] (MOTION_DTYPE, as motion_search_pu_wide returns them for the same planes; only mvx / mvy are
        read) -> (out_nodes, out_pus, out_pus_small) of MOTION_QPEL_DTYPE in the same layouts, None for a family not given (at least one must be)."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        ins, outs, p = self._refine_families(nodes, pus, pus_small)
        self._check(self.lib.fhevc_motion_refine_pu_wide(self.h, cur, ref, stride, qp, max_range, *p))
        return self._per_ctu(outs)

    def motion_refine_pu_wide_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_nodes=None, d_out_nodes=None, d_pus=None, d_out_pus=None,
                                     d_pus_small=None, d_out_pus_small=None, rows=None, stream=None, qp=32, max_range=64):
        """frames 1.. of the batch, each refined in the frame before it, max_range 1..64, around the vectors of d_nodes / d_pus / d_pus_small (what
        motion_search_pu_wide_device wrote for the same rows; 85 / 124 / 384 per CTU); the outputs hold as many quarter-sample entries (16 B).  Each
        family's pair may be None together (not all three).  Asynchronous; keeps no state between calls."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_motion_refine_pu_wide_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp, max_range,
                                                                d_nodes, d_out_nodes, d_pus, d_out_pus, d_pus_small, d_out_pus_small, stream))

    def p_depth_range_device(self, d_nodes, d_prev_maps, num_pictures, d_depth_min, d_depth_max=None, rows=None, stream=None, qp=32,
                             prev_mode="colocated", rule=None):
        """config 4 on the device: the depth ranges of num_pictures P pictures from d_nodes (what motion_search_device wrote for the same rows)
        and d_prev_maps (num_pictures whole-picture maps, numCtus * 256 bytes each); d_depth_min / d_depth_max: num_pictures * band CTUs * 256
        bytes.  prev_mode: "colocated", "unit", "node" or a P_PREV_* value; rule: a PRule (None: the shipped one).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_p_depth_range_device(self.h, d_nodes, d_prev_maps, num_pictures, rb, re, qp, P_PREV.get(prev_mode, prev_mode),
                                                        C.byref(rule) if rule is not None else None, d_depth_min, d_depth_max, stream))

    def p_predict_frame(self, cur_plane, ref_plane, prev_map, origin=0, stride=None, qp=32, search_range=4, prev_mode="colocated", rule=None):
        """config 4, one picture pair from host buffers: motion search of cur in ref (as motion_search) and the depth ranges decided on the
        device against prev_map [numCtus, 256], the reference picture's depths -> (depth_min, depth_max), each [numCtus, 256]."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        prev = np.ascontiguousarray(prev_map, np.uint8).reshape(-1)
        assert prev.size == self.num_ctus * 256
        dmin, dmax = np.zeros(self.num_ctus * 256, np.uint8), np.zeros(self.num_ctus * 256, np.uint8)
        self._check(self.lib.fhevc_p_predict_frame(self.h, cur, ref, stride, qp, search_range,
                                                   prev.ctypes.data, P_PREV.get(prev_mode, prev_mode), C.byref(rule) if rule is not None else None,
                                                   dmin.ctypes.data, dmax.ctypes.data))
        return dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256)

    def pu_shape_select_device(self, d_nodes, d_pus, d_pus_small, num_pictures, d_shapes, d_costs=None, rows=None, stream=None, rule=None):
        """config 4 on the device: the partition-size records of num_pictures P pictures from their refined entries (what motion_refine_pu_wide_device
        wrote for the same rows: 85 / 124 / 384 per CTU; d_pus_small may be None); d_shapes: num_pictures * band CTUs * 85 records (16 B), d_costs
        (optional): ... * 85 * 8 uint32.  rule: a PuShapeRule (None: the unfitted default).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_pu_shape_select_device(self.h, d_nodes, d_pus, d_pus_small, num_pictures, rb, re, C.byref(rule) if rule is not None else None,
                                                          d_shapes, d_costs, stream))

    def pu_shape_select_merge_device(self, d_nodes, d_pus, d_pus_small, d_merge_pus, d_merge_pus_small, num_pictures, d_shapes, d_costs=None, d_merged=None, rows=None,
                                     stream=None, rule=None):
        """pu_shape_select_device with the merge records of motion_merge_pu_device beside the refined PUs (124 / 384 per CTU, compact over the same rows;
        d_merge_pus_small may be None); d_merged (optional): num_pictures * band CTUs * 85 uint16.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_pu_shape_select_merge_device(self.h, d_nodes, d_pus, d_pus_small, d_merge_pus, d_merge_pus_small, num_pictures, rb, re,
                                                                C.byref(rule) if rule is not None else None, d_shapes, d_costs, d_merged, stream))

    def p_shape_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=64, rule=None):
        """config 4, one picture pair from host buffers: the wide SAD search of all three families, their quarter-sample refinement and the partition-size
        selection on the device -> [numCtus, 85] SHAPE_DTYPE; only the records come back."""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        out = np.zeros(self.num_ctus * NODES_PER_CTU, SHAPE_DTYPE)
        self._check(self.lib.fhevc_p_shape_frame(self.h, cur, ref, stride, qp, search_range,
                                                 C.byref(rule) if rule is not None else None, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def p_tree_select_device(self, d_shapes, num_pictures, d_depth_min=None, d_depth_max=None, d_tree=None, rows=None, stream=None, rule=None):
        """config 4 on the device: the depth ranges of num_pictures P pictures from the selection's records (what pu_shape_select_device wrote for the same
        rows: 85 per CTU), decided bottom-up over the quad-tree; d_depth_min / d_depth_max: num_pictures * band CTUs * 256 bytes, d_tree: ... * 85 records
        (16 B); each may be None, not all three.  rule: a PTreeRule (None: the unfitted default).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_p_tree_select_device(self.h, d_shapes, num_pictures, rb, re, C.byref(rule) if rule is not None else None, d_depth_min,
                                                        d_depth_max, d_tree, stream))

    def p_tree_select_merge_device(self, d_shapes, d_merge, num_pictures, d_depth_min=None, d_depth_max=None, d_tree=None, rows=None, stream=None, rule=None):
        """p_tree_select_device with the merge records of motion_merge_device beside the selection's (85 per CTU, compact over the same rows).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_p_tree_select_merge_device(self.h, d_shapes, d_merge, num_pictures, rb, re, C.byref(rule) if rule is not None else None,
                                                              d_depth_min, d_depth_max, d_tree, stream))

    def p_tree_select_skip_device(self, d_shapes, d_merge, d_skip, skip_mask, num_pictures, d_depth_min=None, d_depth_max=None, d_tree=None, rows=None, stream=None,
                                  rule=None):
        """p_tree_select_merge_device with the skip records of motion_skip_device (85 per CTU, compact over the same rows) and skip_mask 0..3.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_p_tree_select_skip_device(self.h, d_shapes, d_merge, d_skip, skip_mask, num_pictures, rb, re,
                                                             C.byref(rule) if rule is not None else None, d_depth_min, d_depth_max, d_tree, stream))

    def p_tree_select_rd_device(self, d_rd_explicit, d_rd_merge, skip_mask, num_pictures, d_depth_min=None, d_depth_max=None, d_tree=None, rows=None, stream=None,
                                rule=None):
        """p_tree_select_skip_device on the RD records of two motion_rd_device launches (85 per CTU, compact over the same rows).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_p_tree_select_rd_device(self.h, d_rd_explicit, d_rd_merge, skip_mask, num_pictures, rb, re,
                                                           C.byref(rule) if rule is not None else None, d_depth_min, d_depth_max, d_tree, stream))

    def p_tree_select_rd_pu_device(self, d_rd_pu, d_rd_merge, skip_mask, num_pictures, d_depth_min=None, d_depth_max=None, d_tree=None, rows=None, stream=None,
                                   rule=None):
        """p_tree_select_rd_device with the folded records of motion_rd_pu_device where d_rd_explicit stands.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_p_tree_select_rd_pu_device(self.h, d_rd_pu, d_rd_merge, skip_mask, num_pictures, rb, re,
                                                              C.byref(rule) if rule is not None else None, d_depth_min, d_depth_max, d_tree, stream))

    def p_tree_select_intra_device(self, d_shapes, d_merge, d_skip, skip_mask, d_intra, num_pictures, d_depth_min=None, d_depth_max=None, d_tree=None, rows=None,
                                   stream=None, rule=None):
        """p_tree_select_skip_device with the intra records of intra_p_device (85 per CTU, compact over the same rows): a node that is not calm takes its
        intra cost where that is strictly smaller.  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_p_tree_select_intra_device(self.h, d_shapes, d_merge, d_skip, skip_mask, d_intra, num_pictures, rb, re,
                                                              C.byref(rule) if rule is not None else None, d_depth_min, d_depth_max, d_tree, stream))

    def intra_p_device(self, num_pictures, d_first, d_first4, d_out, rows=None, stream=None, qp=32):
        """config 4 on the device: the intra candidate costs of num_pictures P pictures from the records of intra_first_pass_device (85 per CTU) and, unless
        None, of intra_first_pass_4x4_device (256 per CTU); d_out: num_pictures * band CTUs * 85 records (16 B).  Asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_intra_p_device(self.h, num_pictures, rb, re, qp, d_first, d_first4, d_out, stream))

    def intra_p(self, first, first4=None, qp=32):
        """one picture, host arrays: first [numCtus, 85], first4 [numCtus, 256] or None (NODE_DTYPE) -> [numCtus, 85] INTRA_P_DTYPE"""
        first = np.ascontiguousarray(first)
        first4 = None if first4 is None else np.ascontiguousarray(first4)
        assert first.size == self.num_ctus * NODES_PER_CTU and first.dtype.itemsize == 16
        assert first4 is None or (first4.size == self.num_ctus * PUS4_PER_CTU and first4.dtype.itemsize == 16)
        out = np.zeros(self.num_ctus * NODES_PER_CTU, INTRA_P_DTYPE)
        self._check(self.lib.fhevc_intra_p(self.h, qp, first.ctypes.data, first4.ctypes.data if first4 is not None else None, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU)

    def p_tree_intra_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None, skip_mask=3,
                           with_shapes=False, with_merge=False, with_intra=False):
        """p_tree_amvp_frame with the zero-residual stage, the two intra first passes of the current picture and the intra stage behind the selection, and the
        tree that takes them -> (depth_min, depth_max) [numCtus, 256], then the records asked for: SHAPE_DTYPE, MOTION_MERGE_DTYPE, INTRA_P_DTYPE [numCtus, 85]"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        dmin, dmax = np.zeros(self.num_ctus * 256, np.uint8), np.zeros(self.num_ctus * 256, np.uint8)
        shapes = np.zeros(self.num_ctus * NODES_PER_CTU, SHAPE_DTYPE) if with_shapes else None
        merge = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_MERGE_DTYPE) if with_merge else None
        intra = np.zeros(self.num_ctus * NODES_PER_CTU, INTRA_P_DTYPE) if with_intra else None
        self._check(self.lib.fhevc_p_tree_intra_frame(self.h, cur, ref, stride, qp, search_range, coarse_range, C.byref(shape_rule) if shape_rule is not None else None,
                                                      C.byref(tree_rule) if tree_rule is not None else None, skip_mask, dmin.ctypes.data, dmax.ctypes.data,
                                                      shapes.ctypes.data if with_shapes else None, merge.ctypes.data if with_merge else None,
                                                      intra.ctypes.data if with_intra else None))
        out = (dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256))
        for a in (shapes, merge, intra):
            out += (a.reshape(self.num_ctus, NODES_PER_CTU),) if a is not None else ()
        return out

    def p_tree_rd_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None, skip_mask=3,
                        with_shapes=False, with_merge=False, with_rd_merge=False, with_rd_pu=False):
        """p_tree_amvp_frame carried to the RD stage: behind the selection the RD estimate of the nodes' merge records, the RD estimates of 2Nx2N and of the
        selection's best and second size folded per node, and the RD tree -> (depth_min, depth_max) [numCtus, 256], then the records asked for [numCtus, 85]:
        SHAPE_DTYPE, MOTION_MERGE_DTYPE, MOTION_RD_DTYPE (of the merge records), MOTION_RD_PU_DTYPE (folded)"""
        return self.p_tree_rd_qt_frame(cur_plane, ref_plane, None, origin, stride, qp, search_range, coarse_range, shape_rule, tree_rule, skip_mask, with_shapes,
                                       with_merge, with_rd_merge, with_rd_pu)

    def p_tree_rd_qt_frame(self, cur_plane, ref_plane, tu_depths=3, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None,
                           skip_mask=3, with_shapes=False, with_merge=False, with_rd_merge=False, with_rd_pu=False):
        """p_tree_rd_frame with all four RD launches at tu_depths TU depths (2: p_tree_rd_frame's bytes; None: the entry point without the argument)"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        dmin, dmax = np.zeros(self.num_ctus * 256, np.uint8), np.zeros(self.num_ctus * 256, np.uint8)
        wanted = ((with_shapes, SHAPE_DTYPE), (with_merge, MOTION_MERGE_DTYPE), (with_rd_merge, MOTION_RD_DTYPE), (with_rd_pu, MOTION_RD_PU_DTYPE))
        arrays = [np.zeros(self.num_ctus * NODES_PER_CTU, dt) if want else None for want, dt in wanted]
        head = (self.h, cur, ref, stride, qp, search_range, coarse_range, C.byref(shape_rule) if shape_rule is not None else None,
                C.byref(tree_rule) if tree_rule is not None else None, skip_mask)
        tail = (dmin.ctypes.data, dmax.ctypes.data, *[a.ctypes.data if a is not None else None for a in arrays])
        self._check(self.lib.fhevc_p_tree_rd_frame(*head, *tail) if tu_depths is None else self.lib.fhevc_p_tree_rd_qt_frame(*head, tu_depths, *tail))
        out = (dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256))
        for a in arrays:
            out += (a.reshape(self.num_ctus, NODES_PER_CTU),) if a is not None else ()
        return out

    def p_tree_rd_intra_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None, skip_mask=3,
                              with_shapes=False, with_merge=False, with_rd_merge=False, with_rd_pu=False, with_first=False):
        """p_tree_rd_frame with the intra candidate: behind the folded inter records the first pass of the current picture and intra_rd gated and folded in
        place, then the RD tree -> (depth_min, depth_max) [numCtus, 256], then the records asked for [numCtus, 85]: p_tree_rd_frame's four and NODE_DTYPE"""
        return self.p_tree_rd_intra_qt_frame(cur_plane, ref_plane, None, origin, stride, qp, search_range, coarse_range, shape_rule, tree_rule, skip_mask, with_shapes,
                                             with_merge, with_rd_merge, with_rd_pu, with_first)

    def p_tree_rd_intra_qt_frame(self, cur_plane, ref_plane, tu_depths=3, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None,
                                 skip_mask=3, with_shapes=False, with_merge=False, with_rd_merge=False, with_rd_pu=False, with_first=False):
        """p_tree_rd_intra_frame with every RD launch, the intra stage included, at tu_depths TU depths (2: p_tree_rd_intra_frame's bytes; None: the entry point
        without the argument)"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        dmin, dmax = np.zeros(self.num_ctus * 256, np.uint8), np.zeros(self.num_ctus * 256, np.uint8)
        wanted = ((with_shapes, SHAPE_DTYPE), (with_merge, MOTION_MERGE_DTYPE), (with_rd_merge, MOTION_RD_DTYPE), (with_rd_pu, MOTION_RD_PU_DTYPE), (with_first, NODE_DTYPE))
        arrays = [np.zeros(self.num_ctus * NODES_PER_CTU, dt) if want else None for want, dt in wanted]
        head = (self.h, cur, ref, stride, qp, search_range, coarse_range, C.byref(shape_rule) if shape_rule is not None else None,
                C.byref(tree_rule) if tree_rule is not None else None, skip_mask)
        tail = (dmin.ctypes.data, dmax.ctypes.data, *[a.ctypes.data if a is not None else None for a in arrays])
        self._check(self.lib.fhevc_p_tree_rd_intra_frame(*head, *tail) if tu_depths is None else self.lib.fhevc_p_tree_rd_intra_qt_frame(*head, tu_depths, *tail))
        out = (dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256))
        for a in arrays:
            out += (a.reshape(self.num_ctus, NODES_PER_CTU),) if a is not None else ()
        return out

    def p_tree_rd_intra_nxn_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None, skip_mask=3,
                                  with_shapes=False, with_merge=False, with_rd_merge=False, with_rd_pu=False, with_first=False, with_nxn=False):
        """p_tree_rd_intra_qt_frame at 3 with the 4x4 first pass of the current picture behind the first pass and intra_rd_nxn in intra_rd_qt's place ->
        that call's results, then (with_nxn) the NxN records [numCtus, 64] INTRA_RD_NXN_DTYPE"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        dmin, dmax = np.zeros(self.num_ctus * 256, np.uint8), np.zeros(self.num_ctus * 256, np.uint8)
        wanted = ((with_shapes, SHAPE_DTYPE), (with_merge, MOTION_MERGE_DTYPE), (with_rd_merge, MOTION_RD_DTYPE), (with_rd_pu, MOTION_RD_PU_DTYPE), (with_first, NODE_DTYPE))
        arrays = [np.zeros(self.num_ctus * NODES_PER_CTU, dt) if want else None for want, dt in wanted]
        nxn = np.zeros(self.num_ctus * NXN_PER_CTU, INTRA_RD_NXN_DTYPE) if with_nxn else None
        self._check(self.lib.fhevc_p_tree_rd_intra_nxn_frame(self.h, cur, ref, stride, qp, search_range, coarse_range, C.byref(shape_rule) if shape_rule is not None else None,
                                                             C.byref(tree_rule) if tree_rule is not None else None, skip_mask, dmin.ctypes.data, dmax.ctypes.data,
                                                             *[a.ctypes.data if a is not None else None for a in arrays], nxn.ctypes.data if with_nxn else None))
        out = (dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256))
        for a in arrays:
            out += (a.reshape(self.num_ctus, NODES_PER_CTU),) if a is not None else ()
        return out + ((nxn.reshape(self.num_ctus, NXN_PER_CTU),) if with_nxn else ())

    def p_tree_rd_intra_search_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None, rule=None,
                                     skip_mask=3, with_shapes=False, with_merge=False, with_rd_merge=False, with_rd_pu=False, with_first=False, with_nxn=False):
        """p_tree_rd_intra_nxn_frame with both first passes' lists (8 candidates) and intra_rd_search under rule (None: the default) in intra_rd_nxn's place ->
        that call's results"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        dmin, dmax = np.zeros(self.num_ctus * 256, np.uint8), np.zeros(self.num_ctus * 256, np.uint8)
        wanted = ((with_shapes, SHAPE_DTYPE), (with_merge, MOTION_MERGE_DTYPE), (with_rd_merge, MOTION_RD_DTYPE), (with_rd_pu, MOTION_RD_PU_DTYPE), (with_first, NODE_DTYPE))
        arrays = [np.zeros(self.num_ctus * NODES_PER_CTU, dt) if want else None for want, dt in wanted]
        nxn = np.zeros(self.num_ctus * NXN_PER_CTU, INTRA_RD_NXN_DTYPE) if with_nxn else None
        self._check(self.lib.fhevc_p_tree_rd_intra_search_frame(self.h, cur, ref, stride, qp, search_range, coarse_range, C.byref(shape_rule) if shape_rule is not None else None,
                                                                C.byref(tree_rule) if tree_rule is not None else None, C.byref(rule) if rule is not None else None, skip_mask,
                                                                dmin.ctypes.data, dmax.ctypes.data, *[a.ctypes.data if a is not None else None for a in arrays],
                                                                nxn.ctypes.data if with_nxn else None))
        out = (dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256))
        for a in arrays:
            out += (a.reshape(self.num_ctus, NODES_PER_CTU),) if a is not None else ()
        return out + ((nxn.reshape(self.num_ctus, NXN_PER_CTU),) if with_nxn else ())

    def p_tree_merge_pu_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None,
                              with_shapes=False, with_merge=False):
        """p_tree_merge_frame with the merge stage per PU behind the one per node, and the selection on merge-aware costs; the same results"""
        return self._p_tree_merge_frame(self.lib.fhevc_p_tree_merge_pu_frame, cur_plane, ref_plane, origin, stride, qp, search_range, coarse_range, shape_rule,
                                        tree_rule, with_shapes, with_merge)

    def p_tree_amvp_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None,
                          with_shapes=False, with_merge=False):
        """p_tree_merge_pu_frame with the re-pricing against neighbour predictors between the refinements and the merge stages; the same results"""
        return self._p_tree_merge_frame(self.lib.fhevc_p_tree_amvp_frame, cur_plane, ref_plane, origin, stride, qp, search_range, coarse_range, shape_rule,
                                        tree_rule, with_shapes, with_merge)

    def p_tree_merge_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None,
                           with_shapes=False, with_merge=False):
        """p_tree_frame with the merge stage between refinement and tree -> (depth_min, depth_max) [numCtus, 256], then the records [numCtus, 85] SHAPE_DTYPE
        (with_shapes) and [numCtus, 85] MOTION_MERGE_DTYPE (with_merge)"""
        return self._p_tree_merge_frame(self.lib.fhevc_p_tree_merge_frame, cur_plane, ref_plane, origin, stride, qp, search_range, coarse_range, shape_rule, tree_rule,
                                        with_shapes, with_merge)

    def _p_tree_merge_frame(self, entry, cur_plane, ref_plane, origin, stride, qp, search_range, coarse_range, shape_rule, tree_rule, with_shapes, with_merge):
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        dmin, dmax = np.zeros(self.num_ctus * 256, np.uint8), np.zeros(self.num_ctus * 256, np.uint8)
        shapes = np.zeros(self.num_ctus * NODES_PER_CTU, SHAPE_DTYPE) if with_shapes else None
        merge = np.zeros(self.num_ctus * NODES_PER_CTU, MOTION_MERGE_DTYPE) if with_merge else None
        self._check(entry(self.h, cur, ref, stride, qp, search_range, coarse_range, C.byref(shape_rule) if shape_rule is not None else None,
                          C.byref(tree_rule) if tree_rule is not None else None, dmin.ctypes.data, dmax.ctypes.data, shapes.ctypes.data if with_shapes else None,
                          merge.ctypes.data if with_merge else None))
        out = (dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256))
        out += (shapes.reshape(self.num_ctus, NODES_PER_CTU),) if with_shapes else ()
        return out + ((merge.reshape(self.num_ctus, NODES_PER_CTU),) if with_merge else ())

    def p_tree_frame(self, cur_plane, ref_plane, origin=0, stride=None, qp=32, search_range=8, coarse_range=0, shape_rule=None, tree_rule=None, with_shapes=False):
        """config 4, one picture pair from host buffers: coarse_range 0: the wide SAD search of all three families, their quarter-sample refinement, the
        partition-size selection and the tree decision on the device; coarse_range 1..14: the same chain around one coarse centre per CTU (search_range
        1..8) -> (depth_min, depth_max) [numCtus, 256]; with_shapes: (depth_min, depth_max, records [numCtus, 85] SHAPE_DTYPE)"""
        cur, ref, stride = self._pair(cur_plane, ref_plane, origin, stride)
        dmin, dmax = np.zeros(self.num_ctus * 256, np.uint8), np.zeros(self.num_ctus * 256, np.uint8)
        shapes = np.zeros(self.num_ctus * NODES_PER_CTU, SHAPE_DTYPE) if with_shapes else None
        self._check(self.lib.fhevc_p_tree_frame(self.h, cur, ref, stride, qp, search_range, coarse_range,
                                                C.byref(shape_rule) if shape_rule is not None else None, C.byref(tree_rule) if tree_rule is not None else None,
                                                dmin.ctypes.data, dmax.ctypes.data, shapes.ctypes.data if with_shapes else None))
        out = (dmin.reshape(self.num_ctus, 256), dmax.reshape(self.num_ctus, 256))
        return out + (shapes.reshape(self.num_ctus, NODES_PER_CTU),) if with_shapes else out

    def intra_first_pass_all(self, plane, origin=0, stride=None, qp=32):
        """(best [numCtus, 85], all [numCtus, 85, 35]): every mode's SATD and cost per node (parity entry point)"""
        flat = np.ascontiguousarray(plane).reshape(-1)
        stride = stride if stride is not None else plane.shape[-1]
        best = np.zeros(self.num_ctus * NODES_PER_CTU, NODE_DTYPE)
        allm = np.zeros(self.num_ctus * NODES_PER_CTU * 35, NODE_DTYPE)
        self._check(self.lib.fhevc_intra_first_pass_all(self.h, flat.ctypes.data + 2 * origin, stride, qp, best.ctypes.data, allm.ctypes.data))
        return best.reshape(self.num_ctus, NODES_PER_CTU), allm.reshape(self.num_ctus, NODES_PER_CTU, 35)

    def intra_first_pass_candidates(self, plane, origin=0, stride=None, qp=32, num_candidates=8):
        """[numCtus, 85, num_candidates] uint8: per node the modes of smallest first-pass cost, best first (HM's candidate list)"""
        flat = np.ascontiguousarray(plane).reshape(-1)
        stride = stride if stride is not None else plane.shape[-1]
        out = np.zeros(self.num_ctus * NODES_PER_CTU * num_candidates, np.uint8)
        self._check(self.lib.fhevc_intra_first_pass_candidates(self.h, flat.ctypes.data + 2 * origin, stride, qp, num_candidates, out.ctypes.data))
        return out.reshape(self.num_ctus, NODES_PER_CTU, num_candidates)

    def intra_first_pass_4x4(self, plane, origin=0, stride=None, qp=32, num_candidates=8):
        """The first pass of the 4x4 PUs of NxN CUs: (best [numCtus, 256] NODE_DTYPE, modes [numCtus, 256, num_candidates] uint8), PUs in raster
        16x16 order per CTU; PUs whose 8x8 CU crosses the picture edge carry mode 255"""
        flat = np.ascontiguousarray(plane).reshape(-1)
        stride = stride if stride is not None else plane.shape[-1]
        best = np.zeros(self.num_ctus * PUS4_PER_CTU, NODE_DTYPE)
        modes = np.zeros(self.num_ctus * PUS4_PER_CTU * num_candidates, np.uint8)
        self._check(self.lib.fhevc_intra_first_pass_4x4(self.h, flat.ctypes.data + 2 * origin, stride, qp, num_candidates, best.ctypes.data, modes.ctypes.data))
        return best.reshape(self.num_ctus, PUS4_PER_CTU), modes.reshape(self.num_ctus, PUS4_PER_CTU, num_candidates)

    def intra_first_pass_4x4_all(self, plane, origin=0, stride=None, qp=32):
        """all [numCtus, 256, 35]: every mode's SATD and cost per 4x4 PU (parity entry point)"""
        flat = np.ascontiguousarray(plane).reshape(-1)
        stride = stride if stride is not None else plane.shape[-1]
        allm = np.zeros(self.num_ctus * PUS4_PER_CTU * 35, NODE_DTYPE)
        self._check(self.lib.fhevc_intra_first_pass_4x4_all(self.h, flat.ctypes.data + 2 * origin, stride, qp, allm.ctypes.data))
        return allm.reshape(self.num_ctus, PUS4_PER_CTU, 35)

    def aq_layout(self, max_aq_depth):
        """Offsets of the AQ layers in the concatenated activity array (max_aq_depth + 1 entries)."""
        off = (C.c_longlong * (max_aq_depth + 1))()
        n = self.lib.fhevc_aq_parts(self.width, self.height, max_aq_depth, off)
        self._check(min(n, 0))
        return list(off)

    def preanalyze(self, plane, origin=0, stride=None, max_aq_depth=3):
        """TEncPreanalyzer::xPreanalyze: (activity of all layers concatenated, per-layer averages)."""
        flat = np.ascontiguousarray(plane).reshape(-1)
        stride = stride if stride is not None else plane.shape[-1]
        off = self.aq_layout(max_aq_depth)
        act = np.zeros(off[-1], np.float64)
        avg = np.zeros(max_aq_depth, np.float64)
        self._check(self.lib.fhevc_preanalyze(self.h, flat.ctypes.data + 2 * origin, stride, max_aq_depth,
                                              act.ctypes.data, avg.ctypes.data))
        return act, avg

    def aq_qp(self, activity, avg_activity, qp_adaptation_range=6, base_qp=32):
        """TEncCu::xComputeQP for every AQ part (host side; no device work)."""
        activity = np.ascontiguousarray(activity, np.float64)
        avg_activity = np.ascontiguousarray(avg_activity, np.float64)
        out = np.zeros(activity.size, np.int8)
        self._check(self.lib.fhevc_aq_qp(activity.ctypes.data, avg_activity.ctypes.data, self.width, self.height,
                                         avg_activity.size, qp_adaptation_range, base_qp, 6 * (self.bit_depth - 8),
                                         out.ctypes.data))
        return out

    def preanalyze_frames_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_activity,
                                 max_aq_depth=3, rows=None, stream=None):
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_preanalyze_frames_device(self.h, d_luma, sample_bytes, stride, frame_stride,
                                                            num_frames, rb, re, max_aq_depth, d_activity, stream))

    def intra_first_pass_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_out, rows=None,
                                stream=None, qp=32):
        """d_out: device buffer of num_frames * band CTUs * 85 NODE_DTYPE entries (16 bytes each); asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_intra_first_pass_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames,
                                                           rb, re, qp, d_out, stream))

    def intra_first_pass_4x4_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_best=None, d_modes=None, rows=None,
                                    stream=None, qp=32, num_candidates=8):
        """d_best: device buffer of num_frames * band CTUs * 256 NODE_DTYPE entries, d_modes: num_frames * band CTUs * 256 * num_candidates
        bytes; either may be None, not both; asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_intra_first_pass_4x4_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames,
                                                               rb, re, qp, num_candidates, d_best, d_modes, stream))

    def intra_first_pass_candidates_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_modes, rows=None,
                                           stream=None, qp=32, num_candidates=8):
        """d_modes: device buffer of num_frames * band CTUs * 85 * num_candidates bytes (intra_first_pass_candidates per picture); asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_intra_first_pass_candidates_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames,
                                                                      rb, re, qp, num_candidates, d_modes, stream))

    def predict_frames_device(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_depth, d_hadamard=None,
                              d_logits=None, rows=None, stream=None, qp=32, d_flags=None):
        """All pointers are raw device addresses (e.g. torch.Tensor.data_ptr()); asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_predict_frames_device(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames,
                                                         rb, re, qp, d_depth, d_hadamard, d_logits, d_flags, stream))

    def predict_frames_device_range(self, d_luma, sample_bytes, stride, frame_stride, num_frames, d_depth, d_depth_max=None, d_hadamard=None,
                                    d_logits=None, rows=None, stream=None, qp=32, d_flags=None, margin_split=0, margin_stop=0):
        """predict_frames_device with soft decisions: d_depth receives depth_min, d_depth_max (optional) depth_max; asynchronous."""
        rb, re = rows if rows is not None else (0, self.ctus_y)
        self._check(self.lib.fhevc_predict_frames_device_range(self.h, d_luma, sample_bytes, stride, frame_stride, num_frames, rb, re, qp,
                                                               margin_split, margin_stop, d_depth, d_depth_max, d_hadamard, d_logits, d_flags, stream))

    def expand_depth_flags_device(self, d_flags, num_frames, d_depth, stream=None):
        self._check(self.lib.fhevc_expand_depth_flags_device(self.h, d_flags, num_frames, d_depth, stream))

    def set_motion_distortion(self, mode):
        """"satd" (default) or "sad" (HM's integer-search distortion: results equal the reference's xPatternSearch)"""
        self._check(self.lib.fhevc_set_motion_distortion(self.h, {"satd": 0, "sad": 1}[mode]))

    def set_cnn_arith(self, arith):
        """"i8" (default) or "f16": the arithmetic of the classifier's conv2 / conv3; the results are the same integers"""
        self._check(self.lib.fhevc_set_cnn_arith(self.h, CNN_ARITH[arith]))

    @property
    def cnn_arith(self):
        v = self.lib.fhevc_get_cnn_arith(self.h)
        return {8: "i8", 16: "f16"}[v]

    def enable_kernel_timing(self, on=True):
        self._check(self.lib.fhevc_enable_kernel_timing(self.h, 1 if on else 0))

    def kernel_timing(self, which, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.lib.fhevc_kernel_timing(self.h, which, 1 if reset else 0, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def stats(self):
        s = Stats()
        self._check(self.lib.fhevc_get_stats(self.h, C.byref(s), C.sizeof(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}
