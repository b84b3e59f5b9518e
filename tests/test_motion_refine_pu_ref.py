"""Pins tests/motion_refine_pu_ref.py, the numpy restatement the PU refinement kernel is held to (no GPU needed): on a square it is the node
restatement; the distortion takes xGetHADs' branch by the PU's sides (4x4 Hadamards over the WHOLE block when a side is no multiple of 8, which
is not the node's 8x8 value minus the other part); two half-sample motions inside one CU are found exactly by the two parts and not by the
square; ties go to the centre; index maps and markers are the searches'."""
import numpy as np
import pytest

import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
from fasthevc_amd import capi
from test_motion_refine_ref import flat_plane, textured


def low_bits(pic, bd, seed):
    """the low bd - 8 bits populated, so that shifting per tile and shifting once differ"""
    return (pic & ~((1 << (bd - 8)) - 1)) | np.random.default_rng(seed).integers(0, 1 << (bd - 8), size=pic.shape)


@pytest.mark.parametrize("bd,qp", [(8, 22), (10, 32), (12, 4)])
def test_on_a_square_it_is_the_node_restatement(oracle, bd, qp):
    W, H = 128, 128
    ref, cur = textured(W, H, bd, 31), textured(W, H, bd, 32)
    planes = mr.Planes(ref, bd, 16)
    flat, org, stride = flat_plane(cur)
    sl = mr.sqrt_lambda(oracle, qp, bd)
    rng = np.random.default_rng(bd)
    for n, x0, y0 in ((64, 64, 0), (32, 32, 96), (16, 112, 16), (8, 120, 120), (8, 0, 0)):
        mx, my = (int(v) for v in rng.integers(-8, 9, size=2))
        assert rp.refine_block(oracle, planes, flat, org, stride, x0, y0, n, n, mx, my, sl) == mr.refine_node(oracle, planes, flat, org, stride, x0, y0, n, mx, my, sl)


def tiled(oracle, planes, flat, stride, q, x0, y0, w, h, t):
    """the unshifted sum of fho_satd over the t x t tiles of block (x0, y0, w, h) at the candidate q (quarter samples): bit depth 8 = no shift, so
    each tile contributes xCalcHADs8x8's (sum + 2) >> 2 or xCalcHADs4x4's (sum + 1) >> 1"""
    s = 0
    for y in range(y0, y0 + h, t):
        for x in range(x0, x0 + w, t):
            s += int(oracle.fho_satd(flat.ctypes.data + 2 * (y * stride + x), stride, planes.block_ptr(q[0], q[1], x, y), planes.width, t, t, 8))
    return s


# (node x0, y0, n), this part (x, y, w, h) and the other part, relative to the node
SMALL_PARTS = [((16, 32, 16), (0, 4, 16, 12), (0, 0, 16, 4)), ((48, 16, 16), (4, 0, 12, 16), (0, 0, 4, 16)), ((32, 48, 16), (0, 12, 16, 4), (0, 0, 16, 12)),
               ((0, 16, 16), (12, 0, 4, 16), (0, 0, 12, 16)), ((40, 8, 8), (0, 4, 8, 4), (0, 0, 8, 4)), ((56, 56, 8), (4, 0, 4, 8), (0, 0, 4, 8))]


def test_a_side_of_4_or_12_goes_wholly_through_4x4_hadamards(oracle):
    bd, qp = 10, 30
    ref, cur = low_bits(textured(96, 96, bd, 41), bd, 1), low_bits(textured(96, 96, bd, 42), bd, 2)
    planes = mr.Planes(ref, bd, 16)
    flat, org, stride = flat_plane(cur)
    sl = mr.sqrt_lambda(oracle, qp, bd)
    differ = 0
    for (nx, ny, n), (px, py, w, h), (ox, oy, ow, oh) in SMALL_PARTS:
        r = rp.refine_block(oracle, planes, flat, org, stride, nx + px, ny + py, w, h, 2, -3, sl)
        for qx, qy, satd, cost in r["half"] + r["quarter"]:
            assert satd == tiled(oracle, planes, flat, stride, (qx, qy), nx + px, ny + py, w, h, 4) >> (bd - 8), (w, h, qx, qy)
            assert cost == satd + mr.qpel_cost(qx, qy, sl)
            if (qx & 3) and (qy & 3):     # a candidate with both fractions: the node's 8x8-tiled value minus the other part is another number
                wrong = (tiled(oracle, planes, flat, stride, (qx, qy), nx, ny, n, n, 8) - tiled(oracle, planes, flat, stride, (qx, qy), nx + ox, ny + oy, ow, oh, 4)) >> (bd - 8)
                differ += wrong != satd
    assert differ >= 4 * len(SMALL_PARTS)


def test_sides_that_are_multiples_of_8_go_through_8x8_hadamards(oracle):
    bd, qp = 10, 30
    ref, cur = low_bits(textured(128, 96, bd, 43), bd, 3), low_bits(textured(128, 96, bd, 44), bd, 4)
    planes = mr.Planes(ref, bd, 16)
    flat, org, stride = flat_plane(cur)
    sl = mr.sqrt_lambda(oracle, qp, bd)
    differ = 0
    for x0, y0, w, h in ((32, 8, 32, 8), (64, 0, 64, 48), (8, 64, 8, 16), (40, 48, 24, 32)):
        r = rp.refine_block(oracle, planes, flat, org, stride, x0, y0, w, h, -1, 4, sl)
        for qx, qy, satd, _ in r["half"] + r["quarter"]:
            assert satd == tiled(oracle, planes, flat, stride, (qx, qy), x0, y0, w, h, 8) >> (bd - 8), (w, h, qx, qy)
            differ += satd != tiled(oracle, planes, flat, stride, (qx, qy), x0, y0, w, h, 4) >> (bd - 8)
    assert differ > 0


@pytest.mark.parametrize("fa,fb", [((2, 0), (0, 2)), ((0, 2), (2, 2)), ((2, 2), (2, 0))])
def test_two_half_sample_motions_inside_one_cu(oracle, fa, fb):
    """part 0 of every CU is the reference at integer vector a plus the half-sample offset fa, part 1 at b plus fb: fed the integer vectors, both
    parts of the shape end at exactly their quarter-unit vectors with nothing left, where the 2Nx2N node keeps a residual"""
    bd, qp, a, b = 10, 4, (2, -1), (-3, 2)
    kinds = list(rp.TWO_MOTION_KINDS)
    ref = textured(64 * len(kinds), 64, bd, 51)
    planes = mr.Planes(ref, bd, 16)
    qa, qb = (4 * a[0] + fa[0], 4 * a[1] + fa[1]), (4 * b[0] + fb[0], 4 * b[1] + fb[1])
    cur = rp.two_motion_picture(planes, kinds, qa, qb)
    flat, org, stride = flat_plane(cur)
    sl = mr.sqrt_lambda(oracle, qp, bd)
    out = {fam: rp.expected(oracle, cur, ref, bd, qp, rp.two_motion_inputs(kinds, fam, a, b), 8, fam, planes=planes) for fam in ("pu", "small")}
    index = {"pu": mp.pu_index, "small": ps.pu_small_index}
    for ctu, kind in enumerate(kinds):
        fam, shape, nodes, _ = rp.TWO_MOTION_KINDS[kind]
        for k in nodes:
            p0, p1 = out[fam][ctu, index[fam](k, shape, 0)], out[fam][ctu, index[fam](k, shape, 1)]
            assert (int(p0["mvx"]), int(p0["mvy"])) == qa and (int(p1["mvx"]), int(p1["mvy"])) == qb, (kind, k)
            assert p0["satd_best"] == 0 and p1["satd_best"] == 0 and p0["satd_int"] > 0 and p1["satd_int"] > 0, (kind, k)
            assert p0["cost_best"] == mr.qpel_cost(*qa, sl) and p1["cost_best"] == mr.qpel_cost(*qb, sl)
            x0, y0, n = mp.node_rect(k)
            for v in (a, b):       # one vector for the whole CU, from either part's integer vector
                assert mr.refine_node(oracle, planes, flat, org, stride, 64 * ctu + x0, y0, n, v[0], v[1], sl)["satd_best"] > 0, (kind, k)


def test_ties_go_to_the_centre(oracle):
    """a flat picture: every candidate has distortion 0.  At QP 0 the quarter stage's four axis neighbours of (0, 0) cost as little as the centre
    (four bits against two, both below one unit of cost), and strict "<" keeps the centre, which comes first; at QP 30 the centre is the cheapest
    outright"""
    bd = 8
    pic = np.full((64, 64), 90, np.int64)
    planes = mr.Planes(pic, bd, 16)
    flat, org, stride = flat_plane(pic)
    for qp, tie in ((0, True), (30, False)):
        sl = mr.sqrt_lambda(oracle, qp, bd)
        for x0, y0, w, h in ((0, 0, 16, 4), (16, 4, 16, 12), (36, 0, 12, 16), (8, 8, 4, 8), (0, 16, 64, 16), (32, 0, 8, 32)):
            r = rp.refine_block(oracle, planes, flat, org, stride, x0, y0, w, h, 0, 0, sl)
            assert (r["mvx"], r["mvy"], r["satd_best"], r["satd_int"]) == (0, 0, 0, 0)
            for stage in ("half", "quarter"):
                assert all(c[2] == 0 for c in r[stage]) and r[stage][0][:2] == (0, 0)
            costs = [c[3] for c in r["quarter"]]
            assert (costs.count(min(costs)) > 1) == tie and costs[0] == min(costs) == r["cost_best"]


def test_index_maps_and_markers(oracle):
    """entries are in the order of the two searches' index maps; a PU of a node that crosses the picture edge carries the marker, and so does a PU
    whose vector is longer than max_range"""
    assert [mp.pu_index(*c) for c in mp.covered()] == list(range(124)) and [capi.motion_pu_index(*c) for c in mp.covered()] == list(range(124))
    assert [ps.pu_small_index(*c) for c in ps.covered()] == list(range(384)) and [capi.motion_pu_small_index(*c) for c in ps.covered()] == list(range(384))
    W, H, bd = 96, 64, 8           # two CTUs; the second is 32 samples wide
    ref, cur = textured(W, H, bd, 1), textured(W, H, bd, 2)
    for fam, covered in (("pu", mp.covered()), ("small", ps.covered())):
        pus = np.zeros((2, len(covered)), capi.MOTION_DTYPE)
        pus["mvx"][0, 3], pus["mvy"][0, 7], pus["mvx"][0, 9] = 5, -5, 4
        got = rp.expected(oracle, cur, ref, bd, 30, pus, 4, fam)
        marked = got["cost_best"] == rp.MARKER
        assert marked[0].sum() == 2 and marked[0, 3] and marked[0, 7] and not marked[0, 9]
        inside = np.array([mp.node_rect(k)[0] + mp.node_rect(k)[2] <= 32 for k, _, _ in covered])
        assert np.array_equal(marked[1], ~inside) and inside.any() and (~inside).any()
        for k in ("satd_int", "satd_best"):
            assert (got[k][marked] == rp.MARKER).all() and (got[k][~marked] != rp.MARKER).all()
        assert (got["mvx"][marked] == 0).all() and (got["mvy"][marked] == 0).all()
        # a valid entry is the block restatement on the PU's own rectangle
        i = 9
        k, s, p = covered[i]
        x0, y0, w, h = mp.pu_rect(k, s, p)
        flat, org, stride = flat_plane(cur)
        r = rp.refine_block(oracle, mr.Planes(ref, bd, 12), flat, org, stride, x0, y0, w, h, 4, 0, mr.sqrt_lambda(oracle, 30, bd))
        assert tuple(got[0, i]) == (r["satd_int"], r["satd_best"], r["cost_best"], r["mvx"], r["mvy"])


def test_planes_of_the_ctus_surroundings_give_what_whole_picture_planes_give(oracle):
    """expected() interpolates only the surroundings of each CTU; with the fractional planes of the whole picture the result is the same, at the
    picture's corners and in its middle, with vectors up to the range"""
    W, H, bd, R = 200, 168, 10, 8
    ref, cur = textured(W, H, bd, 61), textured(W, H, bd, 62)
    whole = mr.Planes(ref, bd, R + 8)
    rng = np.random.default_rng(6)
    for fam, per in (("pu", 124), ("small", 384)):
        pus = np.zeros((12, per), capi.MOTION_DTYPE)
        pus["mvx"], pus["mvy"] = rng.integers(-R, R + 1, size=(12, per)), rng.integers(-R, R + 1, size=(12, per))
        pus["mvx"][:, ::7], pus["mvy"][:, 1::7] = R, -R
        ctus = [0, 3, 5, 8, 11]
        a, b = rp.expected(oracle, cur, ref, bd, 27, pus, R, fam, ctus=ctus), rp.expected(oracle, cur, ref, bd, 27, pus, R, fam, ctus=ctus, planes=whole)
        assert a.tobytes() == b.tobytes() and (a["cost_best"][ctus] != rp.MARKER).any()
