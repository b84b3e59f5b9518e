"""Expected values of the 4x4 first pass (fhevc_intra_first_pass_4x4*), built from the CPU oracle: fho_first_pass_node at n = 4 for every valid
PU of the CTUs asked for, lists by a stable sort on satd + bits * sqrt_lambda.  Not a test module: tests/test_oracle_first_pass_4x4.py pins it
without a GPU, tests/test_gpu_first_pass_4x4.py compares the library with it."""
import ctypes as C
import math

import numpy as np

from fasthevc_amd import capi
from oracle import oracle_py as op

PUS = 256
MODE_BITS = np.array([2, 3] + [6] * 24 + [3] + [6] * 8, np.float64)   # planar 2; DC and vertical (26) 3; the rest 6


def sqrt_lambda(oracle, qp, bd):
    return math.sqrt(oracle.fho_lambda_intra(qp, bd))


def pu_valid(W, H, cx, cy, ux, uy):
    """HM codes NxN only in whole 8x8 CUs: the PU is valid iff the 8x8 block that holds it lies inside the picture"""
    return 64 * cx + 8 * (ux // 2) + 8 <= W and 64 * cy + 8 * (uy // 2) + 8 <= H


def expected(oracle, flat, org, stride, W, H, bd, qp, ctus=None):
    """flat / org / stride: an int16 plane as frames.guarded_plane lays it out (poison=None).  ctus: CTU raster indices (default: all).
    -> dict: best [n, 256] NODE_DTYPE, all [n, 256, 35] NODE_DTYPE, modes [n, 256, 8] uint8 (take [..., :k] for shorter lists)"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    ctus = list(range(cw * ch)) if ctus is None else list(ctus)
    sl = sqrt_lambda(oracle, qp, bd)
    n = len(ctus)
    best = np.zeros((n, PUS), capi.NODE_DTYPE)
    allm = np.zeros((n, PUS, 35), capi.NODE_DTYPE)
    modes = np.full((n, PUS, 8), 255, np.uint8)
    best["satd"], best["mode"], best["cost"] = 0xFFFFFFFF, 255, -1.0
    allm["satd"], allm["mode"], allm["cost"] = 0xFFFFFFFF, 255, -1.0
    nc, satd = op.NodeCost(), np.zeros(35, np.uint32)
    for i, c in enumerate(ctus):
        cx, cy = c % cw, c // cw
        for pu in range(PUS):
            ux, uy = pu % 16, pu // 16
            if not pu_valid(W, H, cx, cy, ux, uy):
                continue
            oracle.fho_first_pass_node(op.ptr(flat, org), stride, W, H, 64 * cx + 4 * ux, 64 * cy + 4 * uy, 4, bd, sl, C.byref(nc), C.c_void_p(satd.ctypes.data))
            cost = satd.astype(np.float64) + MODE_BITS * sl
            best[i, pu] = (nc.satd, nc.mode, nc.cost)
            allm["satd"][i, pu], allm["mode"][i, pu], allm["cost"][i, pu] = satd, np.arange(35), cost
            modes[i, pu] = np.argsort(cost, kind="stable")[:8]
    return dict(best=best, all=allm, modes=modes)
