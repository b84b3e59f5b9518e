"""tests/golden/ref_transform.npz: what the REFERENCE's own forward transform xTrMxN (TComTrQuant.cpp:860-915) returns for blocks of residuals of
8x8, 16x16 and 32x32 samples at bit depths 8, 10 and 12 -- the file the restatement tests/motion_skip_ref.py, and through it fhevc_motion_skip, is
pinned to (tests/test_motion_skip_ref.py, without a GPU).  Per size and bit depth: random residuals over the full range +-(2^bd - 1), the two constant
blocks, the full-swing checkerboards and row / column stripes, single impulses at the four corners, and the residual of one real predicted node
(a pan clip, tests/motion_refine_ref.py's prediction at a quarter-sample vector).  Beside them the six g_quantScales, read from the library's data,
and the three DCT matrices, recovered from the function itself: an impulse of 2^(2 log2 N + bd - 9) at column x of row 0 leaves exactly M[k][x] in
row 0 of the coefficients (the first stage gives M[k][x] 2^(log2 N), the second multiplies by M[0][0] = 64 and shifts by log2 N + 6).

The call is preceded by the reference's initROM, which fills the table the shifts are read from.

CPU only; needs oracle/_ref (python __graft_entry__.py builds it where the reference's sources are).  Integers only:

    python tests/quality/gen_transform_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import motion_refine_ref as mr  # noqa: E402
import oracle_py as op  # noqa: E402
from fasthevc_amd import frames  # noqa: E402

SIZES, DEPTHS = (8, 16, 32), (8, 10, 12)
RANDOM = {8: 6, 16: 4, 32: 2}          # few 32x32 cases: the file stays in the range of the other goldens
OUT = os.path.join(ROOT, "tests", "golden", "ref_transform.npz")


def bind(lib):
    f = getattr(lib, "_Z6xTrMxNiPiS_iibi")       # Void xTrMxN(Int, TCoeff*, TCoeff*, Int, Int, Bool, const Int); TCoeff is Int in this build
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_bool, C.c_int]
    f.restype = None
    getattr(lib, "_Z7initROMv")()                # initROM: the shifts come from g_aucConvertToBit, which it fills

    def transform(block, bd):
        n = block.shape[0]
        src = np.ascontiguousarray(block, np.int32)
        dst = np.zeros((n, n), np.int32)
        f(bd, src.ctypes.data, dst.ctypes.data, n, n, False, 15)
        return dst
    return transform


def blocks(n, bd, rng):
    """-> [(name, block [n, n] int32)]"""
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:n, 0:n]
    out = [(f"random{i}", rng.integers(-top, top + 1, size=(n, n))) for i in range(RANDOM[n])]
    out += [("const+", np.full((n, n), top)), ("const-", np.full((n, n), -top))]
    out += [("checker+", np.where((xx + yy) & 1, -top, top)), ("checker-", np.where((xx + yy) & 1, top, -top))]
    out += [("rows", np.where(yy & 1, -top, top)), ("cols", np.where(xx & 1, -top, top))]
    for name, (y, x) in (("tl", (0, 0)), ("tr", (0, n - 1)), ("bl", (n - 1, 0)), ("br", (n - 1, n - 1))):
        b = np.zeros((n, n), np.int64)
        b[y, x] = top if (x + y) % 2 == 0 else -top
        out.append(("impulse_" + name, b))
    # one real predicted node: pictures 0 and 1 of a pan clip, the node at (64, 64), a quarter-sample vector near the pan's
    ys = frames.pan_clip(176, 144, 2, seed=31 + bd, v_structure=3, v_noise=-2)
    ref, cur = (y.astype(np.int64) << (bd - 8) for y in ys)
    if bd > 8:
        cur = cur + np.random.default_rng(bd).integers(0, 1 << (bd - 8), size=cur.shape)
        ref = ref + np.random.default_rng(bd + 1).integers(0, 1 << (bd - 8), size=ref.shape)
    planes = mr.Planes(ref, bd, 16)
    out.append(("real", cur[64:64 + n, 64:64 + n] - planes.block(-11, 6, 64, 64, n).astype(np.int64)))
    return [(name, np.asarray(b, np.int32)) for name, b in out]


def main():
    ref = op.load_ref()
    transform = bind(ref)
    out = {"quant_scales": np.array((C.c_int * 6).in_dll(ref, "g_quantScales"), np.int32)}
    rng = np.random.default_rng(2264)
    for n in SIZES:
        # the matrix through the function, at every bit depth (the answer must not depend on it)
        recovered = []
        for bd in DEPTHS:
            m = np.zeros((n, n), np.int32)
            for x in range(n):
                b = np.zeros((n, n), np.int32)
                b[0, x] = 1 << (2 * (n.bit_length() - 1) + bd - 9)
                m[:, x] = transform(b, bd)[0, :]
            recovered.append(m)
        assert all((m == recovered[0]).all() for m in recovered)
        out[f"matrix{n}"] = recovered[0]
        for bd in DEPTHS:
            cases = blocks(n, bd, rng)
            out[f"in_{n}_{bd}"] = np.stack([b for _, b in cases]).astype(np.int16)
            out[f"coef_{n}_{bd}"] = np.stack([transform(b, bd) for _, b in cases])
            print(f"N {n} bit depth {bd}: {len(cases)} blocks, largest |coefficient| {int(np.abs(out[f'coef_{n}_{bd}']).max())}")
    out["sizes"], out["depths"] = np.array(SIZES, np.int32), np.array(DEPTHS, np.int32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
