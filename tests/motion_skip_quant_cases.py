"""What the generator of tests/golden/ref_quant.npz (tests/quality/gen_quant_golden.py) and the two tests that read the file (test_motion_skip_quant_pin.py
without a GPU, test_gpu_motion_skip_quant_pin.py on the device) share: the sizes, bit depths and QPs of the file, the clips the real nodes are cut from --
regenerated from frames.pan_clip with fixed seeds and held to a SHA-256 the file stores, never stored themselves --, the layout of a threshold case, and
the coverage the real nodes must reach.  A plain module, not a conftest and not a test."""
import hashlib
import os

import numpy as np

import motion_refine_ref as mr
from fasthevc_amd import frames

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_quant.npz")
SIZES, DEPTHS = (8, 16, 32), (8, 10, 12)
ALL_QPS = tuple(range(52))
NODE_QPS = (0, 22, 27, 32, 37, 51)
RANGES = (8, 16)                      # max_range 8: the kernel's static-LDS instantiation; 16: the dynamic one
W, H, CTUS = 128, 64, 2               # the smallest picture that runs every level's transform mapping and two CTUs through the persistent loop
PAN = 3                               # the clip moves 3 samples per picture: the true vector of every node is (12, 0) quarter samples
TRUE_VECTOR = (4 * PAN, 0)
NOISE = 2                             # amplitude of the uniform noise on the current picture, in 8-bit sample units: what a node at the true vector leaves.
#                                       With 2 the 64x64 nodes quantise to zero from QP 32 on and carry the half bit at QPs 37 and 51; with 3 and 4 too few do
MIN_PAIRS = 8                         # every outcome on at least this many node / QP pairs, per bit depth and level

# ---- (a) threshold cases: K coefficients per (n, bit depth, QP) ------------------------------------------------------------------------------------------
FIXED = (0, 1, -1, 32767, -32767, -32768)
NUM_RANDOM = 238
K = 12 + len(FIXED) + NUM_RANDOM      # 256: four 8x8 blocks, one 16x16 block, the first eight rows of one 32x32 block


def special_values(t_plain, t_half):
    """t - 1, t, t + 1 around both thresholds in both signs, then the fixed values"""
    around = [s * (t + d) for t in (t_plain, t_half) for d in (-1, 0, 1) for s in (1, -1)]
    return np.array(around + list(FIXED), np.int32)


def threshold_blocks(values, n):
    """K coefficients -> [blocks, n, n] int32 in raster order, the tail of the last block zero"""
    per = n * n
    nb = -(-K // per)
    out = np.zeros(nb * per, np.int32)
    out[:K] = values
    return out.reshape(nb, n, n)


def num_blocks(n):
    return -(-K // (n * n))


# ---- (b) the clips -----------------------------------------------------------------------------------------------------------------------------------------

def pictures(bd):
    """-> [reference, current], int64 [H, W] at bd bits: pictures 0 and 1 of a pan clip in which structure and noise move together, cut from the middle
    of a wider clip so that no column wraps; uniform noise of +-NOISE on the current picture; above 8 bit the low bits are populated on both"""
    ys = frames.pan_clip(W + 32, H, 2, seed=77 + bd, v_structure=PAN, v_noise=-PAN)
    ref, cur = (y[:, 16:16 + W].astype(np.int64) for y in ys)
    cur = np.clip(cur + np.random.default_rng(500 + bd).integers(-NOISE, NOISE + 1, size=cur.shape), 0, 255)
    pics = [ref << (bd - 8), cur << (bd - 8)]
    if bd > 8:
        pics = [p + np.random.default_rng(900 + bd + i).integers(0, 1 << (bd - 8), size=p.shape) for i, p in enumerate(pics)]
    return pics


def picture_hash(pics):
    return hashlib.sha256(np.stack(pics).astype("<i2").tobytes()).hexdigest()


def node_rect(ctu, k):
    """-> (level, x0, y0, n) of node k of CTU ctu in the W x H picture"""
    lvl, bx, by = mr.node_geometry(k)
    n = 64 >> lvl
    return lvl, (ctu % (W // 64)) * 64 + bx * n, (ctu // (W // 64)) * 64 + by * n, n


def valid(merge, max_range):
    """[CTUS, 85] bool: the nodes fhevc_motion_skip tests (every node of a 128 x 64 picture is INSIDE)"""
    reach = 4 * max_range + 3
    return (merge["cost_best"] != 0xFFFFFFFF) & (np.abs(merge["mvx"].astype(np.int64)) <= reach) & (np.abs(merge["mvy"].astype(np.int64)) <= reach)


def tus(res):
    """the TUs of a node's residual, min(node, 32) samples wide, in raster order"""
    s = res.shape[0]
    n = min(s, 32)
    return [res[y:y + n, x:x + n] for y in range(0, s, n) for x in range(0, s, n)]


LEVEL_OF = np.array([mr.node_geometry(k)[0] for k in range(85)])


def coverage(plain_zero, half_zero, ok):
    """plain_zero, half_zero, ok: bool [ranges, CTUS, 85, QPs] of one bit depth -> {level: (plain true, plain false, half true, half false)} counted
    over the compared node / QP pairs"""
    out = {}
    for lvl in range(4):
        sel = ok[:, :, LEVEL_OF == lvl]
        p, h = plain_zero[:, :, LEVEL_OF == lvl][sel], half_zero[:, :, LEVEL_OF == lvl][sel]
        out[lvl] = (int(p.sum()), int((~p).sum()), int(h.sum()), int((~h).sum()))
    return out
