"""tests/golden/ref_inverse_transform.npz: what the REFERENCE's own inverse transform xITrMxN (TComTrQuant.cpp:927-990) returns for blocks of
coefficients of 4x4, 8x8, 16x16 and 32x32 at bit depths 8, 10 and 12, what its forward transform xTrMxN returns at 4x4 (which ref_transform.npz
lacks), and its six g_invQuantScales, read from the library's data -- the file the restatement tests/motion_rd_ref.py, and through it fhevc_motion_rd,
is pinned to (tests/test_motion_rd_ref.py, without a GPU).  Per size and bit depth, for the inverse: random coefficients over the full 16-bit range
with +-32767 and -32768 planted, single impulses (of both signs and of the extreme values) at the corners and inside, DC only, blocks whose signs follow
one matrix column so that the first stage runs into its clip (and, through it, the second), and the dequantised levels of one real predicted node (a pan
clip, tests/motion_refine_ref.py's prediction at a quarter-sample vector, quantised at QP 22 by the restatement: only an input).  For the forward 4x4:
gen_transform_golden.py's blocks.

xDeQuant is a member function and xQuant needs a live TU at N = 4; neither is callable through this harness, and what the restatement says of them
rests on the cited lines.

Both calls are preceded by the reference's initROM.  CPU only; needs oracle/_ref (python __graft_entry__.py builds it where the reference's sources are).
Integers only:

    python tests/quality/gen_inverse_transform_golden.py
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

import gen_transform_golden as gt  # noqa: E402
import motion_rd_ref as rd  # noqa: E402
import oracle_py as op  # noqa: E402

SIZES, DEPTHS = (4, 8, 16, 32), (8, 10, 12)
RANDOM = {4: 8, 8: 6, 16: 4, 32: 2}    # few 32x32 cases: the file stays in the range of the other goldens
OUT = os.path.join(ROOT, "tests", "golden", "ref_inverse_transform.npz")


def bind(lib):
    getattr(lib, "_Z7initROMv")()
    sig = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_bool, C.c_int]   # (Int bitDepth, TCoeff*, TCoeff*, Int, Int, Bool useDST, const Int); TCoeff is Int
    fwd, inv = getattr(lib, "_Z6xTrMxNiPiS_iibi"), getattr(lib, "_Z7xITrMxNiPiS_iibi")
    for f in (fwd, inv):
        f.argtypes, f.restype = sig, None

    def call(f, block, bd):
        n = block.shape[0]
        src = np.ascontiguousarray(block, np.int32)
        dst = np.zeros((n, n), np.int32)
        f(bd, src.ctypes.data, dst.ctypes.data, n, n, False, 15)
        return dst
    return (lambda b, bd: call(fwd, b, bd)), (lambda c, bd: call(inv, c, bd))


def coefficient_blocks(n, bd, rng):
    """-> [(name, coefficients [n, n] = [vertical frequency, horizontal frequency])]"""
    m = rd.matrix(n)
    out = []
    for i in range(RANDOM[n]):
        c = rng.integers(-32768, 32768, size=(n, n))
        c.reshape(-1)[rng.choice(n * n, 3, replace=False)] = (32767, -32767, -32768)
        out.append((f"random{i}", c))
    for name, (y, x, v) in (("tl", (0, 0, 32767)), ("tr", (0, n - 1, -32768)), ("bl", (n - 1, 0, -32767)), ("br", (n - 1, n - 1, 32767)), ("mid", (n // 2, 1, 1000)),
                            ("one", (1, n // 2, -1))):
        c = np.zeros((n, n), np.int64)
        c[y, x] = v
        out.append(("impulse_" + name, c))
    for v in (64, -3000):
        c = np.zeros((n, n), np.int64)
        c[0, 0] = v
        out.append((f"dc{v}", c))
    # the signs of matrix column y in every column of coefficients: the first stage's sum for output y is 32767 times the column's absolute sum
    for y, v in ((0, 32767), (n - 1, -32768), (n // 2, 20000)):
        out.append((f"clip{y}", np.repeat((np.sign(m[:, y]) * v)[:, None], n, axis=1)))
    out.append(("clip_second", np.outer(np.sign(m[:, 0]), np.sign(m[:, 1])) * 32767))
    real = dict(gt.blocks(max(n, 8), bd, np.random.default_rng(0)))["real"][:n, :n]
    out.append(("real", rd.dequant(rd.levels(rd.forward(real, bd), n, bd, 22), n, bd, 22)))
    return [(name, np.clip(b, -32768, 32767).astype(np.int32)) for name, b in out]   # -v of v = -32768 is no 16-bit coefficient


def main():
    ref = op.load_ref()
    forward, inverse = bind(ref)
    out = {"inv_quant_scales": np.array((C.c_int * 6).in_dll(ref, "g_invQuantScales"), np.int32)}
    rng = np.random.default_rng(927)
    for n in SIZES:
        for bd in DEPTHS:
            cases = coefficient_blocks(n, bd, rng)
            assert all(b.min() >= -32768 and b.max() <= 32767 for _, b in cases)
            out[f"coef_{n}_{bd}"] = np.stack([b for _, b in cases]).astype(np.int16)
            res = np.stack([inverse(b, bd) for _, b in cases])
            assert res.min() >= -32768 and res.max() <= 32767
            out[f"res_{n}_{bd}"] = res.astype(np.int16)
            print(f"inverse N {n} bit depth {bd}: {len(cases)} blocks, {int((np.abs(res) >= 32767).sum())} samples on the second clip")
    # the 4-point matrix through the forward function, as gen_transform_golden.py recovers the larger ones: at every bit depth the same
    recovered = []
    for bd in DEPTHS:
        m = np.zeros((4, 4), np.int32)
        for x in range(4):
            b = np.zeros((4, 4), np.int32)
            b[0, x] = 1 << (4 + bd - 9)
            m[:, x] = forward(b, bd)[0, :]
        recovered.append(m)
    assert all((m == recovered[0]).all() for m in recovered)
    out["matrix4"] = recovered[0]
    for bd in DEPTHS:
        # gen_transform_golden's blocks need n >= 8 for their real node: its top-left 4x4
        cases = [(name, b[:4, :4]) for name, b in gt.blocks(8, bd, rng)]
        out[f"fwd_in_4_{bd}"] = np.stack([b for _, b in cases]).astype(np.int16)
        out[f"fwd_coef_4_{bd}"] = np.stack([forward(b, bd) for _, b in cases])
        print(f"forward N 4 bit depth {bd}: {len(cases)} blocks, largest |coefficient| {int(np.abs(out[f'fwd_coef_4_{bd}']).max())}")
    out["sizes"], out["depths"] = np.array(SIZES, np.int32), np.array(DEPTHS, np.int32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
