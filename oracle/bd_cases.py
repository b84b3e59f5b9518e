"""Inputs behind tests/golden/ref_bit_depths.npz (oracle/gen_golden.py: bit_depths_golden), regenerated from seeds by the
generator and by the tests alike: the file holds the case lists and the reference's outputs, not the planes.

TEST INFRASTRUCTURE ONLY.  Bit depths 9 to 12 and full-swing samples (0 and 2^bd - 1): the values where a packed 16-bit path,
a `bd - 8` shift or a `1 << (bd - 5)` threshold would go wrong first."""
import numpy as np

from fasthevc_amd import frames

SEED = 20261016

# SATD: the shapes of ref_vectors.npz plus odd even ones; every kind of input at every bit depth
SATD_BIT_DEPTHS = (9, 10, 11, 12)
SATD_SHAPES = ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 4), (4, 8), (16, 8), (8, 16), (32, 8), (16, 4), (2, 2), (6, 6),
               (2, 64), (64, 2), (12, 20))
SATD_KINDS = ("random", "random", "extremes", "zero_vs_max", "max_vs_zero", "basis", "basis")


def hadamard8():
    h = np.array([[1]])
    for _ in range(3):
        h = np.block([[h, h], [h, -h]])
    return h


def satd_pair(bd, w, h, kind, rep):
    """-> (a, b): two 64 x 64 int16 blocks (stride 64) for SATD case (bd, w, h, kind, rep)."""
    hi = (1 << bd) - 1
    rng = np.random.default_rng([SEED, bd, w, h, rep])
    if kind == "random":
        a = rng.integers(0, hi + 1, size=(64, 64))
        b = np.clip(a + rng.normal(0, 12 * (1 << (bd - 8)), size=(64, 64)), 0, hi)
    elif kind == "extremes":
        a, b = (rng.choice(np.array([0, hi]), size=(64, 64)) for _ in range(2))
    elif kind == "zero_vs_max":
        a, b = np.zeros((64, 64)), np.full((64, 64), hi)
    elif kind == "max_vs_zero":
        a, b = np.full((64, 64), hi), np.zeros((64, 64))
    else:  # a Hadamard basis pattern at full swing: the difference puts all its energy into one coefficient
        u, v = rng.integers(0, 8, size=2)
        hm = hadamard8()
        sign = np.outer(hm[v], hm[u])
        a = np.where(np.tile(sign, (8, 8)) > 0, hi, 0)
        b = hi - a
    return np.ascontiguousarray(a, np.int16), np.ascontiguousarray(b, np.int16)


# reference-sample fill and the 35 predictors at the depths ref_vectors.npz lacks
INTRA_BIT_DEPTHS = (9, 11, 12)
INTRA_SIZES = (4, 8, 16, 32, 64)
FILL_REPS = 4


def fill_case(bd, n, rep):
    """-> (picture [2n + 8, 2n + 8] int16 with full-swing samples, availability flags [2 * (2n / 4) + 1] uint8)."""
    hi = (1 << bd) - 1
    rng = np.random.default_rng([SEED, 1, bd, n, rep])
    pic = rng.integers(0, hi + 1, size=(2 * n + 8, 2 * n + 8))
    pic[rng.random(pic.shape) < 0.25] = hi
    pic[rng.random(pic.shape) < 0.1] = 0
    units = 2 * n // 4
    if rep == 0:
        flags = np.ones(2 * units + 1)
    elif rep == 1:
        flags = np.zeros(2 * units + 1)
    else:
        flags = rng.random(2 * units + 1) < 0.5
        if rep == 3:
            flags[:units] = 0  # nothing below / left: the upward search of the padding
    return np.ascontiguousarray(pic, np.int16), np.ascontiguousarray(flags, np.uint8)


def pred_line(bd, n, kind):
    """-> 4n + 1 reference line: "sat" random with saturating samples at both ends of the range, "flat" within a few codes of
    the top of the range (|bl + tl - 2 mid| below this depth's strong-smoothing threshold 2^(bd - 5))."""
    hi = (1 << bd) - 1
    rng = np.random.default_rng([SEED, 2, bd, n, 0 if kind == "sat" else 1])
    if kind == "sat":
        line = rng.integers(0, hi + 1, size=4 * n + 1)
        line[::7] = hi
        line[3::11] = 0
    else:
        line = hi - rng.integers(0, 1 << (bd - 6), size=4 * n + 1)
    return np.ascontiguousarray(line, np.int16)


# initIntraPatternChType on live CUs, built like gen_golden.INTRA_LINE_CASES (content, W x H, bd, qp, CTUs of the 7 x 4 grid)
INTRA_LINE_CASES = (("hetero", 416, 240, 9, 32, (0, 1, 7, 9, 13, 20, 24, 27)), ("hetero", 416, 240, 11, 27, (2, 5, 6, 8, 15, 20, 27)))


def intra_line_plane(content, w, h, bd):
    luma = frames.texture16_luma(w, h) if content == "texture16" else frames.hetero_luma(w, h)
    buf, org, stride = frames.to_pel_plane(luma, bd)
    m = org % stride
    buf[m:m + h, m:m + w] += np.random.default_rng(bd).integers(0, 1 << (bd - 8), (h, w)).astype(np.int16)
    return buf, org, stride


# AQ pre-analysis: (content, W, H, bd, max AQ depth); the flat and checkerboard pictures give the largest sums of squares
PREANALYZE_CASES = (("hetero", 200, 136, 9, 3), ("hetero", 200, 136, 11, 3), ("hetero", 200, 136, 12, 2),
                    ("flat", 128, 64, 9, 2), ("flat", 128, 64, 11, 2), ("flat", 128, 64, 12, 2),
                    ("checker", 128, 64, 9, 2), ("checker", 128, 64, 11, 2), ("checker", 128, 64, 12, 3),
                    ("half", 192, 128, 9, 3), ("half", 192, 128, 11, 3))
AQ_SETTINGS = ((6, 32), (12, 3), (12, -2), (12, -10), (4, 50))  # (QP adaptation range, base QP): the low ones clip at -qp_bd_offset (6 at 9 bit, 18 at 11)


def preanalyze_plane(content, w, h, bd):
    """-> (buffer, origin, stride) of native bd-bit content: "hetero" (frames.native_pel_plane), "flat" 2^bd - 1 everywhere,
    "checker" one-pixel checkerboard of 0 and 2^bd - 1, "half" checkerboard on the left half and 0 on the right."""
    hi = (1 << bd) - 1
    if content == "hetero":
        return frames.native_pel_plane(frames.hetero_luma(w, h), bd, seed=bd)
    buf, org, stride = frames.to_pel_plane(np.zeros((h, w), np.uint8), bd)
    m = org % stride
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "flat":
        v = np.full((h, w), hi)
    else:
        v = ((yy + xx) % 2) * hi
        if content == "half":
            v[:, w // 2:] = 0
    buf[m:m + h, m:m + w] = v
    return buf, org, stride


# xPatternSearch at 9 / 11 bit (native content) and on saturated planes at 10 / 12 bit, 416 x 240:
# (bd, qp, range, content, seed, CTUs of the 7 x 4 grid); content "pan": frames.pan_clip(seed) on native_pel_plane,
# "white_black": the current picture 2^bd - 1 everywhere, the reference 0 (every vector ties on SAD),
# "half_white": the left half white over black, the reference the same shifted 5 samples right
PATTERN_CASES = ((9, 32, 4, "pan", 61, (0, 10, 27)), (9, 30, 64, "pan", 62, (8, 20)),
                 (11, 35, 6, "pan", 63, (3, 13, 24)), (11, 32, 64, "pan", 64, (6, 17)),
                 (10, 32, 4, "white_black", 0, (0, 9)), (12, 37, 64, "white_black", 0, (10,)),
                 (10, 27, 8, "half_white", 0, (2, 3)), (12, 32, 64, "half_white", 0, (3,)))


def pattern_planes(bd, content, seed, w=416, h=240):
    """-> (cur, ref, stride): planes from sample (0, 0) on with HM's stride (W + 160), as gen_golden.pattern_search_golden hands them."""
    hi = (1 << bd) - 1
    if content == "pan":
        ys = frames.pan_clip(w, h, 2, seed=seed, v_structure=7, v_noise=-4)
        (rb, org, stride), (cb, _, _) = (frames.native_pel_plane(y, bd, seed=seed + k) for k, y in enumerate(ys))
    else:
        rb, org, stride = frames.to_pel_plane(np.zeros((h, w), np.uint8), bd)
        cb = rb.copy()
        m = org % stride
        if content == "white_black":
            cb[m:m + h, m:m + w] = hi
        else:
            cb[m:m + h, m:m + w // 2] = hi
            rb[m:m + h, m + 5:m + 5 + w // 2] = hi
    cur = np.ascontiguousarray(cb.reshape(-1)[org:][: (h - 1) * stride + w])
    ref = np.ascontiguousarray(rb.reshape(-1)[org:][: (h - 1) * stride + w])
    return cur, ref, stride
