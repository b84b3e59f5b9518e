"""Config 4 (P slices): the quarter-sample refinements at HM's own SearchRange, fhevc_motion_refine_pu_wide (k_motion_refine.hip for the 85 nodes,
k_motion_refine_pu.hip laid out for vectors up to +-64 for the 508 PUs), on the MI355X: against what the reference itself returned
(tests/golden/ref_frac_search_wide.npz), against the numpy restatements (motion_refine_ref, motion_refine_pu_ref; pinned to that file by
test_oracle_golden_frac_wide.py) and against the existing entry points where they overlap.  Everything on small pictures, bit for bit, every
field, markers included."""
import numpy as np
import pytest

import motion_golden as mg
import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
import motion_refine_wide_cases as wc
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, Guarded, clip_planes, pel, pel_batch, to_dev, torch_cuda  # noqa: F401
from test_motion_refine_ref import textured

pytestmark = pytest.mark.gpu

DT, QDT = capi.MOTION_DTYPE, capi.MOTION_QPEL_DTYPE
FAMS = ("nodes", "pu", "small")
PER = {"nodes": capi.NODES_PER_CTU, "pu": capi.PUS_PER_CTU, "small": capi.PUS_SMALL_PER_CTU}
NODE_OF = {"nodes": np.arange(85), "pu": np.array([k for k, _, _ in mp.covered()]), "small": np.array([k for k, _, _ in ps.covered()])}
W9, H9 = 176, 144      # the ragged picture: 3 x 3 CTUs, the last column 48 wide, the last row 16 tall


def same(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    for k in QDT.names:
        assert np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:5], got[k][got[k] != exp[k]][:5], exp[k][got[k] != exp[k]][:5])


def band_ctus(ctx, rows):
    rows = rows or (0, ctx.ctus_y)
    return (rows[1] - rows[0]) * ctx.ctus_x


def pairs(d_in, g, fams):
    """the six pointer arguments: in / out per family, None for a family not asked for"""
    return [p for f in FAMS for p in ((d_in[f].data_ptr(), g[f].ptr) if f in fams else (None, None))]


def refine_dev(torch, ctx, d_luma_ptr, sb, stride, fs, nf, qp, R, ins, rows=None, stream=None):
    """one call over a device batch; ins: {family: [nf - 1, band CTUs, per CTU]} (a family left out: its pair is NULL) -> {family: the same shape of
    MOTION_QPEL_DTYPE}; guards checked, and the outputs of the families NOT asked for stay untouched"""
    n = band_ctus(ctx, rows)
    d_in = {f: to_dev(torch, a) for f, a in ins.items()}
    g = {f: Guarded(torch, max((nf - 1) * n * PER[f] * 16, 16)) for f in FAMS}
    torch.cuda.synchronize()
    ctx.motion_refine_pu_wide_device(d_luma_ptr, sb, stride, fs, nf, *pairs(d_in, g, ins), rows=rows, stream=stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert all(g[f].untouched() for f in FAMS if f not in ins)
    return {f: g[f].result((nf - 1, n, PER[f])).view(QDT) for f in ins}


def expected_pair(oracle, cur, ref, bd, qp, R, ins, ctus=None):
    """{family: [numCtus, per CTU]} of the restatements for one picture pair; ins: {family: [numCtus, per CTU]}"""
    cur, ref = np.asarray(cur), np.asarray(ref)
    H, W = cur.shape
    planes = mr.Planes(ref, bd, R + 8)
    out = {}
    for f, a in ins.items():
        if f == "nodes":
            out[f] = mr.expected(oracle, np.ascontiguousarray(cur.astype(np.int16)).reshape(-1), 0, W, ref, W, H, bd, qp, a, R, ctus=ctus, planes=planes)
        else:
            out[f] = rp.expected(oracle, cur, ref, bd, qp, a, R, f, ctus=ctus, planes=planes)
    return out


def expected_batch(oracle, pics, bd, qp, R, ins, ctus=None):
    per = [expected_pair(oracle, pics[f], pics[f - 1], bd, qp, R, {k: a[f - 1] for k, a in ins.items()}, ctus=ctus) for f in range(1, len(pics))]
    return {k: np.stack([p[k] for p in per]) for k in ins}


def random_entries(shape, seed, lo, hi):
    """input entries of random bytes with vectors from lo .. hi: nothing but mvx / mvy may matter"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=shape + (16,), dtype=np.uint8).view(DT).reshape(shape)
    a["mvx"], a["mvy"] = rng.integers(lo, hi + 1, size=shape), rng.integers(lo, hi + 1, size=shape)
    return a


def random_ins(nf, n, seed, lo, hi):
    return {f: random_entries((nf - 1, n, PER[f]), seed + i, lo, hi) for i, f in enumerate(FAMS)}


def node_inside(W, H):
    """{family: [numCtus, per CTU] bool}: the entry's CU node lies wholly inside the picture"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    out = {}
    for f in FAMS:
        rect = np.array([mp.node_rect(int(k)) for k in NODE_OF[f]])
        cx, cy = np.arange(cw * ch) % cw, np.arange(cw * ch) // cw
        out[f] = (64 * cx[:, None] + rect[None, :, 0] + rect[None, :, 2] <= W) & (64 * cy[:, None] + rect[None, :, 1] + rect[None, :, 2] <= H)
    return out


# ---- 1. / 2. the reference's own results -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases():
    return wc.wide_frac_cases()


@pytest.mark.parametrize("k", range(11))
def test_golden_host_form_all_families_and_each_alone(cases, k):
    assert len(cases) == 11
    c = cases[k]
    (rb, org, stride), (cb, _, _) = pel(c.ref), pel(c.cur)
    ctx = capi.Context(c.W, c.H, c.bd)
    ins = {f: c.inputs(f, seed=k) for f in FAMS}
    got = dict(zip(FAMS, ctx.motion_refine_pu_wide(cb, rb, org, stride, qp=c.qp, max_range=c.R, nodes=ins["nodes"], pus=ins["pu"], pus_small=ins["small"])))
    for f in FAMS:
        assert mg.same(got[f][c.ctus], c.records(f), (c, f)) == wc.PER_CASE[f]
        alone = ctx.motion_refine_pu_wide(cb, rb, org, stride, qp=c.qp, max_range=c.R, **{{"nodes": "nodes", "pu": "pus", "small": "pus_small"}[f]: ins[f]})
        assert [o is None for o in alone] == [x != f for x in FAMS]
        assert alone[FAMS.index(f)].tobytes() == got[f].tobytes(), (c, f)
    ctx.close()


def test_golden_device_form_on_uint8_planes_between_canaries(cases, torch_cuda):
    torch = torch_cuda
    c8 = [c for c in cases if c.bd == 8]
    done = dict.fromkeys(FAMS, 0)
    for c in c8:
        ctx = capi.Context(c.W, c.H, 8, max_frames=2)
        guard = np.full(4096, CANARY, np.uint8)
        flat = np.concatenate([guard, np.stack([c.ref, c.cur]).astype(np.uint8).reshape(-1), guard])
        d_luma = to_dev(torch, flat)
        ins = {f: c.inputs(f, seed=3)[None] for f in FAMS}
        got = refine_dev(torch, ctx, d_luma.data_ptr() + 4096, 1, c.W, c.W * c.H, 2, c.qp, c.R, ins)
        for f in FAMS:
            done[f] += mg.same(got[f][0][c.ctus], c.records(f), (c, f))
        for f in FAMS:   # each family alone: the others' outputs stay untouched (checked inside refine_dev)
            assert refine_dev(torch, ctx, d_luma.data_ptr() + 4096, 1, c.W, c.W * c.H, 2, c.qp, c.R, {f: ins[f]})[f].tobytes() == got[f].tobytes(), (c, f)
        ctx.close()
    assert len(c8) >= 6 and done == {f: len(c8) * n for f, n in wc.PER_CASE.items()}


# ---- 3. the wide search and its refinement on one stream ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("R,speeds", [(9, (9, -9)), (33, (19, -27)), (64, (40, -51))])
def test_search_and_refinement_on_one_stream_without_a_host_synchronisation(oracle, torch_cuda, bd, R, speeds):
    torch = torch_cuda
    qp = 20 + bd + R // 8
    ys = frames.pan_clip(W9, H9, 2, seed=bd + R, v_structure=speeds[0], v_noise=speeds[1])
    pics = clip_planes(ys, bd, low_bits_seed=R)
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W9, H9, bd, max_frames=2)
    n = ctx.num_ctus
    d_luma = to_dev(torch, flat)
    lp = d_luma.data_ptr() + 2 * org
    st = torch.cuda.Stream()
    mid = {f: Guarded(torch, n * PER[f] * 16) for f in FAMS}
    out = {f: Guarded(torch, n * PER[f] * 16) for f in FAMS}
    torch.cuda.synchronize()
    ctx.motion_search_pu_wide_device(lp, 2, stride, fs, 2, mid["nodes"].ptr, mid["pu"].ptr, mid["small"].ptr, stream=st.cuda_stream, qp=qp, search_range=R)
    ctx.motion_refine_pu_wide_device(lp, 2, stride, fs, 2, mid["nodes"].ptr, out["nodes"].ptr, mid["pu"].ptr, out["pu"].ptr, mid["small"].ptr, out["small"].ptr,
                                     stream=st.cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    vec = {f: mid[f].result((n, PER[f])) for f in FAMS}
    exp = expected_pair(oracle, pics[1], pics[0], bd, qp, R, vec)
    for f in FAMS:
        got = out[f].result((n, PER[f])).view(QDT)
        same(got, exp[f], (bd, R, f))
        valid = got["cost_best"] != mr.MARKER
        assert np.array_equal(valid, vec[f]["cost_best"] != mr.MARKER)
        assert (np.maximum(np.abs(vec[f]["mvx"].astype(np.int64)), np.abs(vec[f]["mvy"].astype(np.int64)))[valid] > 8).any(), (bd, R, f)   # long vectors occurred
    ctx.close()


# ---- 4. two long quarter-sample motions inside one CU ------------------------------------------------------------------------------------------------

def two_motion_ctu(planes, ref, ctu_xy, kind, qa, qb):
    """the reference picture with one CTU replaced: part 0 of every CU of rp.TWO_MOTION_KINDS[kind] holds the reference displaced by qa (quarter
    samples), the rest of the CTU by qb -- samples taken from the fractional planes themselves, so the prediction at the true vector equals them"""
    H, W = ref.shape

    def displaced(q):
        a = planes.planes[q[1] & 3][q[0] & 3]
        y, x = planes.pad + (q[1] >> 2), planes.pad + (q[0] >> 2)
        return a[y:y + H, x:x + W].astype(np.int64)

    yy, xx = np.mgrid[0:64, 0:64]
    sel = (slice(64 * ctu_xy[1], 64 * ctu_xy[1] + 64), slice(64 * ctu_xy[0], 64 * ctu_xy[0] + 64))
    cur = ref.copy()
    cur[sel] = np.where(rp.TWO_MOTION_KINDS[kind][3](xx, yy), displaced(qa)[sel], displaced(qb)[sel])
    return cur


@pytest.mark.parametrize("kind", ["2NxnU@16", "2NxN@32"])
@pytest.mark.parametrize("bd,a,fa,b,fb", [(10, (41, -13), (2, 1), (-27, -35), (3, 2)), (8, (-58, 9), (1, 3), (12, -49), (2, 2)), (12, (9, -57), (3, 3), (-33, 10), (1, 1))])
def test_two_long_quarter_sample_motions_inside_one_cu(oracle, bd, a, fa, b, fb, kind):
    """the centre CTU of the ragged picture, built with the restatement's interpolation of the reference: the 16x4 / 16x12 parts (2NxnU) of every
    16x16 CU, or the halves (2NxN) of every 32x32 CU, each displaced by its own vector with both components beyond 8 samples and non-zero
    fractions (the displaced blocks stay inside the picture: 64 samples to its left and top, 48 to its right, 16 below).  Fed the integer parts,
    both parts end at exactly their quarter-unit vectors with no distortion left"""
    qp, R, ctu = 4, 64, 4
    qa, qb = (4 * a[0] + fa[0], 4 * a[1] + fa[1]), (4 * b[0] + fb[0], 4 * b[1] + fb[1])
    assert min(abs(v) for v in a + b) > 8 and all(fa + fb)
    ref = textured(W9, H9, bd, 51)
    planes = mr.Planes(ref, bd, R + 8)
    cur = two_motion_ctu(planes, ref, (1, 1), kind, qa, qb)
    (rb, org, stride), (cb, _, _) = pel(ref), pel(cur)
    ctx = capi.Context(W9, H9, bd)
    ins = {f: np.zeros((ctx.num_ctus, PER[f]), DT) for f in ("pu", "small")}
    for f in ins:
        ins[f][ctu] = rp.two_motion_inputs([kind], f, a, b)[0]
    none, pus, small = ctx.motion_refine_pu_wide(cb, rb, org, stride, qp=qp, max_range=R, pus=ins["pu"], pus_small=ins["small"])
    out = {"pu": pus, "small": small}
    assert none is None
    for f in ("pu", "small"):
        same(out[f], rp.expected(oracle, cur, ref, bd, qp, ins[f], R, f, planes=planes), f)
    f, shape, nodes, _ = rp.TWO_MOTION_KINDS[kind]
    index = {"pu": capi.motion_pu_index, "small": capi.motion_pu_small_index}[f]
    for k in nodes:
        p0, p1 = out[f][ctu, index(k, shape, 0)], out[f][ctu, index(k, shape, 1)]
        assert (int(p0["mvx"]), int(p0["mvy"])) == qa and (int(p1["mvx"]), int(p1["mvy"])) == qb, (kind, k)
        assert p0["satd_best"] == 0 and p1["satd_best"] == 0 and p0["satd_int"] > 0 and p1["satd_int"] > 0, (kind, k)
    ctx.close()


# ---- 5. overlap with the existing entry points -------------------------------------------------------------------------------------------------------

def existing_dev(torch, ctx, lp, sb, stride, fs, nf, qp, R, ins):
    """fhevc_motion_refine_device for the nodes and fhevc_motion_refine_pu_device for the PUs -> {family: bytes}"""
    n = ctx.num_ctus
    d_in = {f: to_dev(torch, a) for f, a in ins.items()}
    g = {f: Guarded(torch, (nf - 1) * n * PER[f] * 16) for f in ins}
    torch.cuda.synchronize()
    if "nodes" in ins:
        ctx.motion_refine_device(lp, sb, stride, fs, nf, d_in["nodes"].data_ptr(), g["nodes"].ptr, qp=qp, max_range=R)
    if "pu" in ins:
        ctx.motion_refine_pu_device(lp, sb, stride, fs, nf, d_in["pu"].data_ptr(), g["pu"].ptr, d_in["small"].data_ptr(), g["small"].ptr, qp=qp, max_range=R)
    torch.cuda.synchronize()
    return {f: g[f].result((nf - 1, n, PER[f])).tobytes() for f in ins}


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_overlap_with_the_existing_entry_points(torch_cuda, bd):
    """max_range 5 and 8: the bytes of fhevc_motion_refine_pu_device / fhevc_motion_refine_device.  max_range 64 on input vectors within +-8: the bytes of
    those entry points at max_range 8 -- the same arithmetic through the other window, a cross-check that needs no restatement.  The nodes at
    max_range 64 on long vectors: the bytes of fhevc_motion_refine_device at 64"""
    torch = torch_cuda
    NF, qp = 3, 28
    pics = clip_planes(frames.pan_clip(W9, H9, NF, seed=31 + bd, v_structure=3, v_noise=-2), bd, low_bits_seed=2)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    lp = d_luma.data_ptr() + 2 * org
    ctx = capi.Context(W9, H9, bd, max_frames=NF)
    ins = random_ins(NF, ctx.num_ctus, 100 + bd, -8, 8)
    for f in FAMS:     # the window's own corners of the MR = 8 layout, in the corner CTUs
        ins[f]["mvx"][:, 0, ::3], ins[f]["mvy"][:, 0, ::3] = -8, -8
        ins[f]["mvx"][:, 8, ::3], ins[f]["mvy"][:, 8, ::3] = 8, 8
    old8 = existing_dev(torch, ctx, lp, 2, stride, fs, NF, qp, 8, ins)
    for R, ref in ((5, existing_dev(torch, ctx, lp, 2, stride, fs, NF, qp, 5, ins)), (8, old8), (64, old8), (9, old8)):
        got = refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R, ins)
        for f in FAMS:
            assert got[f].tobytes() == ref[f], (R, f)
            assert (got[f]["cost_best"] != mr.MARKER).any()
    wide = {"nodes": random_entries((NF - 1, ctx.num_ctus, 85), 7, -64, 64)}
    assert refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, 64, wide)["nodes"].tobytes() == existing_dev(torch, ctx, lp, 2, stride, fs, NF, qp, 64, wide)["nodes"]
    ctx.close()


def test_whole_window_staging_writes_the_same_bytes(torch_cuda, monkeypatch):
    """FHEVC_REFINE_PU_STAGE=full is read when a context is created: such a context stages the whole 200 x 200 window whatever max_range is and writes
    the bytes the default context writes, which stages the part max_range reaches"""
    torch = torch_cuda
    NF, bd, qp = 2, 10, 31
    pics = clip_planes(frames.pan_clip(W9, H9, NF, seed=77, v_structure=21, v_noise=-30), bd, low_bits_seed=6)
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    lp = d_luma.data_ptr() + 2 * org
    ctx = capi.Context(W9, H9, bd, max_frames=NF)
    monkeypatch.setenv("FHEVC_REFINE_PU_STAGE", "full")
    ctx_full = capi.Context(W9, H9, bd, max_frames=NF)
    monkeypatch.delenv("FHEVC_REFINE_PU_STAGE")
    for R in (9, 10, 11, 12, 33, 64):     # every remainder of (64 - max_range) mod 4: the chunk the part's first column falls into
        ins = random_ins(NF, ctx.num_ctus, R, -R, R)
        for f in FAMS:
            ins[f]["mvx"][:, 0, ::2], ins[f]["mvy"][:, 0, ::2] = -R, -R
            ins[f]["mvx"][:, 8, ::2], ins[f]["mvy"][:, 8, ::2] = R, R
        here, there = (refine_dev(torch, c, lp, 2, stride, fs, NF, qp, R, ins) for c in (ctx, ctx_full))
        for f in FAMS:
            assert there[f].tobytes() == here[f].tobytes(), (R, f)
    ctx.close()
    ctx_full.close()


# ---- 6. validity ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,R,span", [(8, 64, 70), (10, 20, 64), (12, 64, 70)])
def test_random_input_bytes_and_markers(oracle, torch_cuda, bd, R, span):
    """only mvx / mvy of the input are read; the marker appears exactly where the CU node leaves the picture or a component exceeds max_range, instead of
    a read outside the window; the corner CTUs are fed the window's own corners"""
    torch = torch_cuda
    NF, qp = 2, 26
    pics = clip_planes(frames.pan_clip(W9, H9, NF, seed=31, v_structure=3, v_noise=4), bd, low_bits_seed=8)
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W9, H9, bd, max_frames=NF)
    ins = random_ins(NF, ctx.num_ctus, 70 + bd, -span, span)
    for f in FAMS:
        ins[f]["mvx"][:, 0, ::2], ins[f]["mvy"][:, 0, ::2] = -R, -R
        ins[f]["mvx"][:, 8, ::2], ins[f]["mvy"][:, 8, ::2] = R, R
        ins[f]["mvx"][:, 2, ::2], ins[f]["mvy"][:, 2, ::2] = R, -R
        ins[f]["mvx"][:, 6, ::2], ins[f]["mvy"][:, 6, ::2] = -R, R
    d_luma = to_dev(torch, flat)
    got = refine_dev(torch, ctx, d_luma.data_ptr() + 2 * org, 2, stride, fs, NF, qp, R, ins)
    exp = expected_batch(oracle, pics, bd, qp, R, ins)
    inside = node_inside(W9, H9)
    for f in FAMS:
        same(got[f], exp[f], f)
        too_long = (np.abs(ins[f]["mvx"].astype(np.int64)) > R) | (np.abs(ins[f]["mvy"].astype(np.int64)) > R)
        mark = got[f]["cost_best"] == mr.MARKER
        assert np.array_equal(mark, too_long | ~inside[f][None]) and too_long.any() and (~mark).any()
        assert (got[f]["satd_int"][mark] == mr.MARKER).all() and (got[f]["satd_best"][mark] == mr.MARKER).all()
        assert (got[f]["mvx"][mark] == 0).all() and (got[f]["mvy"][mark] == 0).all() and (got[f]["satd_int"][~mark] != mr.MARKER).all()
    ctx.close()


# ---- 7. layouts -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [1, 0], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("dtype,bd", [(np.int16, 10), (np.int16, 12), (np.uint8, 8)])
def test_guarded_planes_poisoned_margins_both_load_paths(oracle, torch_cuda, dtype, bd, shift):
    """nothing outside the picture is read for its value: margins, stride padding and the gap between frames hold poison.  shift 1: odd origin and
    odd stride, no row is aligned (the scalar staging path); shift 0: HM's alignment (the 8-byte / 4-byte staging path).  Outputs between 4 KiB
    canaries are written over exactly their extent (refine_dev)"""
    torch = torch_cuda
    NF, qp, R = 2, 27, 33
    ys = frames.pan_clip(W9, H9, NF, seed=9, v_structure=-14, v_noise=26)
    pics = clip_planes(ys, bd, low_bits_seed=17)
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, extra_stride=3 * shift, shift=shift, frame_gap=5 * shift, poison=77)
    assert (stride % 2 == 1 and origin % 2 == 1) if shift else (stride % 8 == 0 and origin % 8 == 0)
    sb = np.dtype(dtype).itemsize
    ctx = capi.Context(W9, H9, bd, max_frames=NF)
    d_luma = to_dev(torch, flat)
    ins = random_ins(NF, ctx.num_ctus, 90 + bd, -R, R)
    out = refine_dev(torch, ctx, d_luma.data_ptr() + sb * origin, sb, stride, fstride, NF, qp, R, ins)
    exp = expected_batch(oracle, pics, bd, qp, R, ins)
    for f in FAMS:
        same(out[f], exp[f], f)
    ctx.close()


def test_bands_between_canaries_an_empty_band_and_slot_12(torch_cuda):
    torch = torch_cuda
    NF, bd, qp, R = 3, 10, 33, 40
    pics = clip_planes(frames.pan_clip(W9, H9, NF, seed=12, v_structure=9, v_noise=-12), bd, low_bits_seed=4)
    flat, org, stride, fs = pel_batch(pics)
    ctx = capi.Context(W9, H9, bd, max_frames=NF)
    d_luma = to_dev(torch, flat)
    lp = d_luma.data_ptr() + 2 * org
    ins = random_ins(NF, ctx.num_ctus, 5, -R, R)
    whole = refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R, ins)
    cw = ctx.ctus_x
    for rows in ((1, 3), (0, 1), (1, 2)):     # compact over the band, written over exactly its extent (guards checked inside refine_dev)
        band_in = {f: np.ascontiguousarray(ins[f][:, rows[0] * cw:rows[1] * cw]) for f in FAMS}
        got = refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R, band_in, rows=rows)
        for f in FAMS:
            assert got[f].tobytes() == np.ascontiguousarray(whole[f][:, rows[0] * cw:rows[1] * cw]).tobytes(), (rows, f)
    # an empty band writes nothing, launches nothing and succeeds
    d_in = {f: to_dev(torch, ins[f]) for f in FAMS}
    g = {f: Guarded(torch, 4096) for f in FAMS}
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.motion_refine_pu_wide_device(lp, 2, stride, fs, NF, *pairs(d_in, g, FAMS), rows=(2, 2), qp=qp, max_range=R)
    torch.cuda.synchronize()
    assert all(x.untouched() for x in g.values()) and ctx.stats()["kernels_launched"] == launched
    # every launch is counted and timed under which = 12 and under no other slot: one for the nodes, one for the PUs of both families
    ctx.enable_kernel_timing(True)
    for s in (7, 10, 11, 12):
        ctx.kernel_timing(s, reset=True)
    big = {f: Guarded(torch, (NF - 1) * cw * PER[f] * 16) for f in FAMS}
    for fams, count, max_range in ((FAMS, 2, R), (("pu", "small"), 1, R), (("nodes",), 1, R), (("small",), 1, 8), (FAMS, 2, 5)):
        ctx.motion_refine_pu_wide_device(lp, 2, stride, fs, NF, *pairs(d_in, big, fams), rows=(0, 1), qp=qp, max_range=max_range)
        torch.cuda.synchronize()
        ms, got = ctx.kernel_timing(12, reset=True)
        launched += count
        assert got == count and ms > 0.0 and ctx.stats()["kernels_launched"] == launched, (fams, max_range)
        assert all(ctx.kernel_timing(s)[1] == 0 for s in (7, 10, 11))
    # ... and the existing PU refinement still counts under its own slot
    ctx.motion_refine_pu_device(lp, 2, stride, fs, NF, d_in["pu"].data_ptr(), big["pu"].ptr, d_in["small"].data_ptr(), big["small"].ptr, rows=(0, 1), qp=qp, max_range=8)
    torch.cuda.synchronize()
    assert ctx.kernel_timing(10)[1] == 1 and ctx.kernel_timing(12)[1] == 0
    ctx.enable_kernel_timing(False)
    ctx.close()


def test_more_ctus_than_the_persistent_grid(oracle, torch_cuda):
    """22 pictures of 416 x 240 that alternate between two = 21 refinements of 28 CTUs = 588 work items in one launch, more than the two workgroups that
    each of 256 CUs holds.  The inputs alternate too: every odd refinement equals the first, every even one the second; CTUs 0, 13 and 27 of the
    first two are held to the restatement (the last work item of the launch is refinement 21's CTU 27)"""
    torch = torch_cuda
    W, H, NF, qp, R = 416, 240, 22, 32, 64
    ys = frames.pan_clip(W, H, 2, seed=40, v_structure=12, v_noise=-19)
    pics = [ys[f % 2].astype(np.int64) for f in range(NF)]
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    assert (NF - 1) * n > 2 * 256
    two = random_ins(3, n, 11, -R, R)
    ins = {f: np.ascontiguousarray(two[f][np.arange(NF - 1) % 2]) for f in FAMS}
    d_luma = to_dev(torch, np.stack([ys[f % 2] for f in range(NF)]))
    got = refine_dev(torch, ctx, d_luma.data_ptr(), 1, W, W * H, NF, qp, R, ins)
    for f in FAMS:
        for s in range(2, NF - 1):
            assert got[f][s].tobytes() == got[f][s % 2].tobytes(), (f, s)
        assert got[f][0].tobytes() != got[f][1].tobytes()
    ctus = [0, 13, 27]
    for s in (0, 1):
        exp = expected_pair(oracle, pics[s + 1], pics[s], 8, qp, R, {f: ins[f][s] for f in FAMS}, ctus=ctus)
        for f in FAMS:
            same(got[f][s][ctus], exp[f][ctus], (s, f))
    ctx.close()


# ---- 8. streams; 9. the host form; 10. rejected calls -----------------------------------------------------------------------------------------------

def test_two_streams_in_flight_with_different_qps_and_ranges(torch_cuda):
    """calls on two non-blocking streams, no synchronisation between them, different QPs and ranges -- one layout each: each output equals that of its
    own synchronous call (the bit costs travel with the launch; nothing is shared in HBM, nothing is kept in the context)"""
    torch = torch_cuda
    W, H, NF = 416, 240, 3
    pics = [y.astype(np.int64) for y in frames.pan_clip(W, H, NF, seed=21, v_structure=12, v_noise=-25)]
    flat, org, stride, fs = pel_batch(pics)
    d_luma = to_dev(torch, flat)
    lp = d_luma.data_ptr() + 2 * org
    ctx = capi.Context(W, H, 8, max_frames=NF)
    n = ctx.num_ctus
    ins = random_ins(NF, n, 55, -64, 64)
    for f in FAMS:     # half of the vectors within +-5: valid at every range below
        ins[f]["mvx"][..., ::2] //= 13
        ins[f]["mvy"][..., ::2] //= 13
    calls = [(12, 64), (47, 5), (30, 64), (22, 8)]
    alone = [refine_dev(torch, ctx, lp, 2, stride, fs, NF, qp, R, ins) for qp, R in calls]
    assert not np.array_equal(alone[0]["pu"]["cost_best"], alone[2]["pu"]["cost_best"])
    assert all((a[f]["cost_best"] != mr.MARKER).any() for a in alone for f in FAMS)
    d_in = {f: to_dev(torch, ins[f]) for f in FAMS}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [{f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS} for _ in calls]
    torch.cuda.synchronize()
    for i, (qp, R) in enumerate(calls):
        ctx.motion_refine_pu_wide_device(lp, 2, stride, fs, NF, *pairs(d_in, outs[i], FAMS), stream=streams[i % 2].cuda_stream, qp=qp, max_range=R)
    torch.cuda.synchronize()
    for i in range(len(calls)):
        for f in FAMS:
            assert outs[i][f].result(alone[i][f].shape).tobytes() == alone[i][f].tobytes(), (i, f)
    ctx.close()


def test_host_form_equals_device_form(torch_cuda):
    torch = torch_cuda
    qp = 29
    for bd, R in ((8, 64), (10, 33), (12, 12), (10, 8)):
        pics = clip_planes(frames.pan_clip(W9, H9, 2, seed=60 + bd, v_structure=10, v_noise=-9), bd, low_bits_seed=1)
        (rb, org, stride), (cb, _, _) = pel(pics[0]), pel(pics[1])
        ctx = capi.Context(W9, H9, bd)
        ins = random_ins(2, ctx.num_ctus, bd, -R - 2, R + 2)
        host = dict(zip(FAMS, ctx.motion_refine_pu_wide(cb, rb, org, stride, qp=qp, max_range=R, nodes=ins["nodes"][0], pus=ins["pu"][0], pus_small=ins["small"][0])))
        d_luma = to_dev(torch, np.stack([rb, cb]))
        dev = refine_dev(torch, ctx, d_luma.data_ptr() + 2 * org, 2, stride, rb.size, 2, qp, R, ins)
        for f in FAMS:
            assert host[f].tobytes() == dev[f][0].tobytes(), (bd, f)
            assert (host[f]["cost_best"] != mr.MARKER).any() and (host[f]["cost_best"] == mr.MARKER).any()
        # two families: the third comes back as None
        a, b, none = ctx.motion_refine_pu_wide(cb, rb, org, stride, qp=qp, max_range=R, nodes=ins["nodes"][0], pus=ins["pu"][0])
        assert none is None and a.tobytes() == host["nodes"].tobytes() and b.tobytes() == host["pu"].tobytes()
        ctx.close()


def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H = 416, 240
    ctx = capi.Context(W, H, 8)
    ctx10 = capi.Context(W, H, 10)
    n = ctx.num_ctus
    d_luma = torch.zeros((2 * W * H,), dtype=torch.int16, device="cuda")
    d_in = {f: torch.zeros((n * PER[f] * 16,), dtype=torch.uint8, device="cuda") for f in FAMS}
    out = {f: Guarded(torch, n * PER[f] * 16) for f in FAMS}
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, luma=d_luma.data_ptr(), sb=2, stride=W, fs=W * H, nf=2, rb=0, re=ctx.ctus_y, qp=32, mr=64, nodes=d_in["nodes"].data_ptr(), onodes=out["nodes"].ptr,
                pus=d_in["pu"].data_ptr(), opus=out["pu"].ptr, small=d_in["small"].data_ptr(), osmall=out["small"].ptr)
    bad = [dict(luma=None), dict(nodes=None, onodes=None, pus=None, opus=None, small=None, osmall=None), dict(nodes=None), dict(onodes=None), dict(pus=None), dict(opus=None),
           dict(small=None), dict(osmall=None), dict(nodes=None, onodes=None, pus=None, opus=None, osmall=None), dict(pus=None, opus=None, small=None, osmall=None, onodes=None),
           dict(nf=1), dict(nf=0), dict(qp=-1), dict(qp=52), dict(mr=0), dict(mr=65), dict(mr=-8), dict(mr=128),
           dict(stride=W - 1), dict(rb=-1), dict(re=ctx.ctus_y + 1), dict(rb=3, re=2), dict(sb=3), dict(sb=0), dict(ctx=ctx10.h, sb=1)]
    launched = ctx.stats()["kernels_launched"]

    def call(a):
        return lib.fhevc_motion_refine_pu_wide_device(a["ctx"], a["luma"], a["sb"], a["stride"], a["fs"], a["nf"], a["rb"], a["re"], a["qp"], a["mr"], a["nodes"], a["onodes"],
                                                      a["pus"], a["opus"], a["small"], a["osmall"], None)
    for change in bad:
        a = dict(good, **change)
        assert call(a) == capi.E_INVALID, change
        assert len(lib.fhevc_last_error(a["ctx"])) > 0, change          # the context says why
    assert call(dict(good, ctx=None)) == capi.E_INVALID
    torch.cuda.synchronize()
    assert all(x.untouched() for x in out.values()) and ctx.stats()["kernels_launched"] == launched and ctx10.stats()["kernels_launched"] == 0
    # the host form refuses the same way
    z = np.zeros((H, W), np.int16)
    hin = {f: np.zeros((n, PER[f]), DT) for f in FAMS}
    res = {f: np.zeros((n, PER[f]), QDT) for f in FAMS}
    p = lambda a: a.ctypes.data
    full = [p(x) for f in FAMS for x in (hin[f], res[f])]
    for qp, mrange, stride in ((52, 64, W), (-1, 64, W), (32, 0, W), (32, 65, W), (32, 64, W - 1)):
        assert lib.fhevc_motion_refine_pu_wide(ctx.h, p(z), p(z), stride, qp, mrange, *full) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu_wide(ctx.h, p(z), p(z), W, 32, 64, None, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu_wide(ctx.h, p(z), p(z), W, 32, 64, p(hin["nodes"]), None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu_wide(ctx.h, p(z), p(z), W, 32, 64, None, None, None, None, None, p(res["small"])) == capi.E_INVALID
    assert lib.fhevc_motion_refine_pu_wide(ctx.h, None, p(z), W, 32, 64, *full) == capi.E_INVALID
    assert not any(r.view(np.uint8).any() for r in res.values()) and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted and writes the whole extent of all three outputs
    assert call(good) == capi.OK
    torch.cuda.synchronize()
    for f in FAMS:
        assert not (out[f].result((n, PER[f])).view(np.uint8).reshape(-1, 16) == CANARY).all(axis=1).any(), f
    ctx.close()
    ctx10.close()
