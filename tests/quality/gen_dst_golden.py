"""tests/golden/ref_dst.npz: what the REFERENCE's own transforms return for 4x4 blocks with useDST true -- xTrMxN (TComTrQuant.cpp:857-925) and xITrMxN
(:927-990), which then go through fastForwardDst / fastInverseDst (:412-466) and g_as_DST_MAT_4 (TComRom.cpp:513-517) -- at bit depths 8, 10 and 12: the
file the restatement tests/intra_rd_qt_ref.py, and through it fhevc_intra_rd_qt at tu_depths 3, is pinned to (tests/test_intra_rd_qt_ref.py, without a
GPU).  The blocks are gen_inverse_transform_golden.py's families at N = 4 (random coefficients over the full 16-bit range with the extreme values planted,
impulses, DC only, sign patterns that run the first stage into its clip, the dequantised levels of one real node) with the sign patterns of the DST
matrix's columns added, and for the forward transform gen_transform_golden.py's blocks, as that generator uses them.  The impulses among them pin every entry of the matrix.

xQuant / xDeQuant at N = 4 stay on the restatement, as they do for the DCT.  Both calls are preceded by the reference's initROM.  CPU only; needs
oracle/_ref (python __graft_entry__.py builds it where the reference's sources are).  Integers only:

    python tests/quality/gen_dst_golden.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "quality"))

import gen_inverse_transform_golden as gi  # noqa: E402
import gen_transform_golden as gt  # noqa: E402
import oracle_py as op  # noqa: E402

DEPTHS = (8, 10, 12)
OUT = os.path.join(ROOT, "tests", "golden", "ref_dst.npz")


def bind(lib):
    getattr(lib, "_Z7initROMv")()
    sig = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_bool, C.c_int]   # (Int bitDepth, TCoeff*, TCoeff*, Int, Int, Bool useDST, const Int); TCoeff is Int
    fwd, inv = getattr(lib, "_Z6xTrMxNiPiS_iibi"), getattr(lib, "_Z7xITrMxNiPiS_iibi")
    for f in (fwd, inv):
        f.argtypes, f.restype = sig, None

    def call(f, block, bd):
        src = np.ascontiguousarray(block, np.int32)
        dst = np.zeros((4, 4), np.int32)
        f(bd, src.ctypes.data, dst.ctypes.data, 4, 4, True, 15)
        return dst
    return (lambda b, bd: call(fwd, b, bd)), (lambda c, bd: call(inv, c, bd))


def main():
    ref = op.load_ref()
    forward, inverse = bind(ref)
    out = {}
    rng = np.random.default_rng(412)
    for bd in DEPTHS:
        cases = gi.coefficient_blocks(4, bd, rng)
        dst = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]])
        for y, v in ((0, 32767), (3, -32768), (2, 20000)):
            s = np.where(dst[:, y] >= 0, 1, -1) * v
            cases.append((f"dst_clip{y}", np.clip(np.repeat(s[:, None], 4, axis=1), -32768, 32767).astype(np.int32)))
        out[f"coef_{bd}"] = np.stack([b for _, b in cases]).astype(np.int16)
        res = np.stack([inverse(b, bd) for _, b in cases])
        assert res.min() >= -32768 and res.max() <= 32767
        out[f"res_{bd}"] = res.astype(np.int16)
        print(f"inverse DST bit depth {bd}: {len(cases)} blocks, {int((np.abs(res) >= 32767).sum())} samples on the second clip")
        fcases = [(name, b[:4, :4]) for name, b in gt.blocks(8, bd, rng)]
        out[f"fwd_in_{bd}"] = np.stack([b for _, b in fcases]).astype(np.int16)
        out[f"fwd_coef_{bd}"] = np.stack([forward(b, bd) for _, b in fcases])
        print(f"forward DST bit depth {bd}: {len(fcases)} blocks, largest |coefficient| {int(np.abs(out[f'fwd_coef_{bd}']).max())}")
    out["depths"] = np.array(DEPTHS, np.int32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
