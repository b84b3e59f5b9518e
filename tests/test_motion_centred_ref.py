"""The restatement of the coarse motion centres (tests/motion_centred_ref.py) without a GPU: its sliding-window form against the literal
loop over cells and candidates, its lambda and bit counts against the CPU oracle's, and the definition's consequences on constructed content --
a texture panned by a multiple of 4 gives exactly that centre on interior CTUs, a flat picture gives (0, 0), a pan beyond 4 Rc gives what the
definition says (the literal form), a CTU narrower than one cell gets the marker."""
import ctypes as C

import numpy as np
import pytest

import motion_centred_ref as cr

MARKER = cr.MARKER


def same(a, b, what=""):
    for k in cr.DT.names:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


def test_lambda_and_bits_are_the_oracles(oracle):
    for qp in range(52):
        for bd in (8, 10, 12):
            assert cr.sqrt_lambda(qp) == np.sqrt(oracle.fho_lambda_intra(qp, bd)), (qp, bd)
    # the cost of the whole-sample vector 4 d is fho_mv_cost's (getCostOfVectorWithPredictor, zero predictor, iCostScale 2)
    for qp in (0, 22, 37, 51):
        sl = cr.sqrt_lambda(qp)
        vc = cr.vector_costs(cr.MAX_RC, sl)
        for dy in range(-cr.MAX_RC, cr.MAX_RC + 1):
            for dx in range(-cr.MAX_RC, cr.MAX_RC + 1):
                assert vc[dy + cr.MAX_RC, dx + cr.MAX_RC] == oracle.fho_mv_cost(4 * dx, 4 * dy, C.c_double(sl)), (qp, dx, dy)
    assert cr.bits(0) == 1 and cr.bits(4) == cr.bits(-4) == 11 and cr.bits(56) == cr.bits(-56) == 17 and 2 * cr.bits(56) < 40


def test_decimation():
    p = np.arange(11 * 14).reshape(11, 14) * 7 % 256
    d = cr.decimate(p)
    assert d.shape == (2, 3)
    for Y in range(2):
        for X in range(3):
            assert d[Y, X] == (p[4 * Y:4 * Y + 4, 4 * X:4 * X + 4].sum() + 8) >> 4
    assert cr.decimate(np.full((8, 8), 255)).tolist() == [[255, 255], [255, 255]]
    assert cr.decimate(np.zeros((3, 9))).shape == (0, 2)


@pytest.mark.parametrize("W,H,bd,qp,Rc", [(104, 88, 8, 30, 2), (72, 40, 10, 22, 3), (68, 132, 12, 41, 1), (66, 64, 8, 35, 2), (40, 24, 8, 12, 14)])
def test_sliding_window_form_equals_the_literal_form(W, H, bd, qp, Rc):
    rng = np.random.default_rng(W + H + bd)
    cur, ref = cr.panned_pair(W, H, bd, seed=qp, vx=8, vy=-4)
    cur = np.clip(cur + rng.integers(-6, 7, size=cur.shape), 0, (1 << bd) - 1)       # not an exact pan: the distortions are not zero
    sl = cr.sqrt_lambda(qp)
    got = cr.centres(cur, ref, bd, sl, Rc)
    same(got, cr.centres_literal(cur, ref, bd, sl, Rc), (W, H, bd, Rc))
    assert len(got) == ((W + 63) // 64) * ((H + 63) // 64)
    if W == 66:   # the second CTU column is 2 samples wide: no cell, the marker and a zero vector
        assert got[1]["cost_best"] == MARKER and got[1]["satd_zero"] == MARKER and got[1]["satd_best"] == MARKER and got[1]["mvx"] == 0 and got[1]["mvy"] == 0
        assert got[0]["cost_best"] != MARKER
    else:
        assert (got["cost_best"] != MARKER).all()


@pytest.mark.parametrize("bd,qp,v", [(8, 32, (20, -12)), (10, 27, (-24, 4)), (12, 37, (56, -56)), (8, 51, (-56, 56)), (8, 0, (0, 0)), (10, 40, (4, 0))])
def test_a_pan_by_a_multiple_of_4_is_found_exactly_on_interior_ctus(bd, qp, v):
    W, H = 320, 256                      # 5 x 4 CTUs: CTUs (1..3, 1..2) are interior for +-56
    cur, ref = cr.panned_pair(W, H, bd, seed=bd + qp, vx=v[0], vy=v[1])
    sl = cr.sqrt_lambda(qp)
    got = cr.centres(cur, ref, bd, sl, 14).reshape(4, 5)
    inner = got[1:3, 1:4]
    assert (inner["mvx"] == v[0]).all() and (inner["mvy"] == v[1]).all() and (inner["satd_best"] == 0).all()
    assert (inner["cost_best"] == cr.bit_cost(cr.bits(v[0]) + cr.bits(v[1]), sl)).all()
    if v != (0, 0):
        assert (inner["satd_zero"] > inner["cost_best"]).all()
    # a smaller range that still holds the pan finds it too; one that does not returns what the literal form says
    need = max(abs(v[0]), abs(v[1])) // 4
    if 1 <= need < 14:
        g = cr.centres(cur, ref, bd, sl, need).reshape(4, 5)[1:3, 1:4]
        assert (g["mvx"] == v[0]).all() and (g["mvy"] == v[1]).all()


def test_a_pan_beyond_the_range_gives_what_the_definition_says():
    W, H, bd, qp, Rc = 192, 128, 8, 30, 3
    cur, ref = cr.panned_pair(W, H, bd, seed=5, vx=40, vy=-28)      # 10 and 7 cells: outside +-3
    sl = cr.sqrt_lambda(qp)
    got = cr.centres(cur, ref, bd, sl, Rc)
    same(got, cr.centres_literal(cur, ref, bd, sl, Rc))
    assert (np.abs(got["mvx"]) <= 4 * Rc).all() and (np.abs(got["mvy"]) <= 4 * Rc).all() and (got["satd_best"] > 0).all()
    assert (got["mvx"] % 4 == 0).all() and (got["mvy"] % 4 == 0).all()


@pytest.mark.parametrize("bd", [8, 12])
def test_flat_content_lands_on_zero(bd):
    W, H = 176, 144
    flat = np.full((H, W), (1 << bd) - 3, np.int64)
    for qp in (0, 32, 51):
        sl = cr.sqrt_lambda(qp)
        got = cr.centres(flat, flat, bd, sl, 14)
        assert (got["mvx"] == 0).all() and (got["mvy"] == 0).all() and (got["satd_zero"] == 0).all() and (got["satd_best"] == 0).all()
        assert (got["cost_best"] == cr.bit_cost(2, sl)).all()


# ---- the integer searches around a centre ---------------------------------------------------------------------------------------------------------------

import motion_range_sweep as rs  # noqa: E402


def clip_pair(bd):
    p = rs.planes("slow", bd)
    return p[1], p[0]       # (cur, ref) of the 104 x 88 sweep clip


def test_centred_volume_is_the_sub_window_of_the_wide_volume():
    cur, ref = clip_pair(10)
    x0, y0, w, h = 64, 64, 40, 24        # the corner CTU
    wide = rs.sad_volume(cur, ref, x0, y0, w, h)
    for (px, py), R in (((0, 0), 8), ((20, -12), 5), ((-56, 56), 8), ((56, -56), 1), ((-3, 7), 8)):
        sub = wide[:, :, 64 + py - R:64 + py + R + 1, 64 + px - R:64 + px + R + 1]
        assert np.array_equal(cr.centred_volume(cur, ref, x0, y0, w, h, px, py, R), sub), (px, py, R)


@pytest.mark.parametrize("bd", [8, 12])
def test_zero_centres_give_the_existing_restatement(oracle, bd):
    cur, ref = clip_pair(bd)
    qp = rs.clip_qp("slow", bd)
    sweep = rs.PairSweep(oracle, cur, ref, bd, qp, rmax=8)
    for R in (1, 5, 8):
        got = cr.centred_search(oracle, cur, ref, bd, qp, R, cr.make_centres([(0, 0)] * 4))
        for f in cr.FAMS:
            assert got[f].tobytes() == sweep.records(R)[f].tobytes(), (bd, R, f)


def test_centres_out_of_range_mark_their_ctu_and_a_pan_is_found_around_its_centre(oracle):
    W, H, bd, qp, R = 192, 128, 8, 30, 5
    cur, ref = cr.panned_pair(W, H, bd, seed=3, vx=23, vy=-14)
    rng = np.random.default_rng(1)
    cur = cur.copy()
    cur[64:72, 64:72] = rng.integers(0, 256, size=(8, 8))          # one 8x8 node of CTU 4 that matches nowhere
    cen = cr.make_centres([(20, -12), (57, 0), (0, -57), (24, -16), (20, -12), (-56, 56)])
    got = cr.centred_search(oracle, cur, ref, bd, qp, R, cen)
    for f in cr.FAMS:
        assert (got[f][[1, 2]]["cost_best"] == MARKER).all() and (got[f][[1, 2]]["mvx"] == 0).all() and (got[f][[1, 2]]["satd_zero"] == MARKER).all()
        assert (got[f][[0, 3, 4, 5]]["cost_best"] != MARKER).all()
    n4 = got["nodes"][4]          # CTU (1, 1): every read inside the picture
    whole = np.ones(85, bool)
    whole[[0, 1, 5, 21]] = False  # the nodes that hold the replaced 8x8 block
    assert (n4["mvx"][whole] == 23).all() and (n4["mvy"][whole] == -14).all() and (n4["satd_best"][whole] == 0).all()
    sl = cr.sqrt_lambda(qp)
    assert (n4["cost_best"][whole] == cr.bit_cost(cr.bits(3) + cr.bits(-2), sl)).all()       # the cost of d = v - P, not of v
    assert (n4["satd_zero"][whole] > 0).all()                                                  # the SAD at the centre (20, -12)
    v = got["nodes"][5]           # around (-56, 56): vectors stay inside the window
    assert (np.abs(v["mvx"] + 56) <= R).all() and (np.abs(v["mvy"] - 56) <= R).all()


# ---- the quarter-sample refinements around a centre --------------------------------------------------------------------------------------------------------

def test_centred_refinement_with_a_zero_centre_is_the_existing_restatement_and_the_cost_is_rebased(oracle):
    import motion_refine_pu_ref as rp
    import motion_refine_ref as mr
    bd = 10
    cur, ref = clip_pair(bd)
    qp = rs.clip_qp("slow", bd)
    sl = mr.sqrt_lambda(oracle, qp, bd)
    planes = mr.Planes(ref, bd, rs.MAXR + 8)
    flat = np.ascontiguousarray(np.asarray(cur).astype(np.int16)).reshape(-1)
    rng = np.random.default_rng(0)
    for f in cr.FAMS:
        for i in range(0, cr.PER[f], 29):
            _, x0, y0, w, h = rs.ENTRIES[f][i]
            mx, my = (int(v) for v in rng.integers(-8, 9, size=2))
            r = mr.refine_node(oracle, planes, flat, 0, rs.W, x0, y0, w, mx, my, sl) if f == "nodes" else rp.refine_block(oracle, planes, flat, 0, rs.W, x0, y0, w, h, mx, my, sl)
            got = cr.refine_block_centred(oracle, planes, flat, rs.W, x0, y0, w, h, mx, my, 0, 0, sl)
            assert got == (r["satd_int"], r["satd_best"], r["cost_best"], r["mvx"], r["mvy"]), (f, i)
            # around a centre that equals the vector the integer candidate costs two bits, and the distortions are those of the absolute vector
            at = cr.refine_block_centred(oracle, planes, flat, rs.W, x0, y0, w, h, mx, my, mx, my, sl)
            assert at[0] == got[0] and at[2] <= at[0] + cr.bit_cost(2, sl)
    # validity: node inside, centre in range, |mv - P| <= max_range
    ins = {"nodes": np.zeros((4, 85), cr.DT)}
    ins["nodes"]["mvx"][:] = 20
    ins["nodes"]["mvy"][:] = -12
    cen = cr.make_centres([(20, -12), (28, -12), (29, -12), (20, 57)])
    out = cr.centred_refine(oracle, cur, ref, bd, qp, 8, cen, ins, planes=planes)["nodes"]
    assert (out[0]["cost_best"] != MARKER).all()                                     # CTU 0 is whole
    assert (out[1]["cost_best"] != MARKER).sum() == rs.valid_entries(rs.W, rs.H)["nodes"][1].sum()    # |20 - 28| = 8: in range where the node is inside
    assert (out[2]["cost_best"] == MARKER).all() and (out[3]["cost_best"] == MARKER).all() and (out[2]["mvx"] == 0).all()
    assert (np.abs(out[0]["mvx"] - 80) <= 3).all() and (np.abs(out[0]["mvy"] + 48) <= 3).all()        # absolute, quarter units


# ---- the restatements against the reference's own results -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(9))
def test_restatements_vs_the_reference_golden(oracle, k):
    """tests/golden/ref_motion_centred.npz: the reference's xPatternSearch and xPatternSearchFracDIF on the displaced reference picture, which is a search and a
    refinement around the centre with the predictor 4 P for every entry whose reads stay inside the picture; those entries in every field, counted"""
    cases = cr.golden_cases()
    assert len(cases) == 9
    c = cases[k]
    assert {x.bd for x in cases} == {8, 10, 12} and {x.qp for x in cases} == {0, 32, 51} and {x.R for x in cases} == {1, 5, 8}
    assert {int(x.centres["mvx"][i]) % 8 for x in cases for i in x.ctus} == set(range(8))
    got = cr.centred_search(oracle, c.cur, c.ref, c.bd, c.qp, c.R, c.centres, ctus=c.ctus)
    fine = cr.centred_refine(oracle, c.cur, c.ref, c.bd, c.qp, c.R, c.centres, c.full_inputs(), ctus=c.ctus)
    four = c.ctus.index(4)
    for f in cr.FAMS:
        assert cr.same_flagged(got[f][c.ctus], c.search[f], c.inside[f], cr.DT.names, (c, f)) == c.counts[f] > 0
        assert cr.same_flagged(fine[f][c.ctus], c.frac[f], c.inside_frac[f], cr.QDT.names, (c, f)) == c.counts_frac[f] > 0
        # every valid entry of CTU 4 is flagged
        assert (c.inside[f][four] == (got[f][4]["cost_best"] != MARKER)).all() and (c.inside_frac[f][four] == c.inside[f][four]).all()
