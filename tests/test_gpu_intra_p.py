"""Config 4 (P slices): the intra stage (k_intra_p.hip), the tree decision that takes its costs (the intra instantiation of k_p_tree.hip) and the frame chain
that runs everything (fhevc_p_tree_intra_frame) on the MI355X, byte for byte against the Python restatement tests/intra_p_ref.py, which
tests/test_intra_p_ref.py holds to hand-computed cases without a GPU, and against the host twins.  Nothing is compared with a kernel's own output except
where two launches must give the same bytes.

The draw's pictures are 200 x 136 (4 x 3 CTUs) and 100 x 76 (2 x 2), ragged on both sides; real records come from a 100 x 76 picture; the constructed pair is
128 x 64."""
import ctypes as C
import itertools

import numpy as np
import pytest

import intra_p_ref as ip
import p_tree_ref as pt
from fasthevc_amd import capi
from motion_gpu_helpers import CANARY, pel, pel_batch, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

IDT, NDT, TDT = capi.INTRA_P_DTYPE, capi.NODE_DTYPE, capi.TREE_DTYPE
ALL = (True, True, True)
P = ip.DRAW_PICTURES


class Guarded:
    """nbytes of device output between two canary-filled guards of 4 KiB, everything pre-filled with the canary; offset: the payload starts that many
    bytes behind a 16-byte boundary"""
    GUARD = 4096

    def __init__(self, torch, nbytes, offset=0):
        self.n, self.off = int(nbytes), self.GUARD + offset
        self.t = torch.full((self.n + 2 * self.GUARD + 16,), CANARY, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.off

    def result(self, dtype, shape):
        h = self.t.cpu().numpy()
        assert (h[:self.off] == CANARY).all() and (h[self.off + self.n:] == CANARY).all(), "a guard around the output was written"
        return h[self.off:self.off + self.n].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.t.cpu().numpy() == CANARY).all())


def at_offset(torch, a, offset):
    """the bytes of `a` on the device, starting `offset` bytes behind a 16-byte boundary -> (tensor that owns them, pointer)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros((raw.size + 32,), dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[offset:offset + raw.size] = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + offset


def band(a, rows, cw):
    return None if a is None else np.ascontiguousarray(a[:, rows[0] * cw:rows[1] * cw])


def run_stage(torch, ctx, first, first4, qp, rows=None, in_offset=0, in4_offset=0, out_offset=0, stream=None):
    """first [P, band CTUs, 85], first4 [P, band CTUs, 256] or None -> the intra records [P, band CTUs, 85]; the output lies between canaries"""
    held = at_offset(torch, first, in_offset)
    held4 = at_offset(torch, first4, in4_offset) if first4 is not None else (None, None)
    out = Guarded(torch, first.size * 16, out_offset)
    torch.cuda.synchronize()
    ctx.intra_p_device(first.shape[0], held[1], held4[1], out.ptr, rows=rows, stream=stream, qp=qp)
    torch.cuda.synchronize()
    return out.result(IDT, first.shape)


@pytest.fixture(scope="module")
def contexts(torch_cuda):
    c = {size: capi.Context(*size, 8) for size in ip.DRAW_SIZES}
    yield c
    for x in c.values():
        x.close()


# ---- 1. the stage kernel on the draw ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ip.DRAW_SIZES)
def test_stage_on_the_draw_as_one_batch(torch_cuda, contexts, size):
    W, H = size
    ctx, d = contexts[size], ip.draw(size)
    cw, ch = (W + 63) // 64, (H + 63) // 64
    for f4, exp in ((d["first4"], d["out"]), (None, d["out_no4"])):
        got = run_stage(torch_cuda, ctx, d["first"], f4, ip.DRAW_QP)
        ip.same(got, exp, ("whole batch", f4 is None))
        # the host twin gives the same bytes, picture by picture
        for p in (0, P - 1):
            assert capi.intra_p_picture(d["first"][p], None if f4 is None else f4[p], W, H, qp=ip.DRAW_QP).tobytes() == got[p].tobytes()
    # bands, compact over their rows
    for rows in [(a, b) for a in range(ch) for b in range(a + 1, ch + 1)][1:]:
        got = run_stage(torch_cuda, ctx, band(d["first"], rows, cw), band(d["first4"], rows, cw), ip.DRAW_QP, rows=rows)
        ip.same(got, band(d["out"], rows, cw), rows)
    # the empty band launches nothing and writes nothing
    held, held4, out = to_dev(torch_cuda, d["first"]), to_dev(torch_cuda, d["first4"]), Guarded(torch_cuda, 4096)
    launched = ctx.stats()["kernels_launched"]
    ctx.intra_p_device(P, held.data_ptr(), held4.data_ptr(), out.ptr, rows=(1, 1), qp=ip.DRAW_QP)
    torch_cuda.cuda.synchronize()
    assert out.untouched() and ctx.stats()["kernels_launched"] == launched
    # another QP on the same records
    ip.same(run_stage(torch_cuda, ctx, d["first"][:2], d["first4"][:2], 51), ip.stage(d["first"][:2], d["first4"][:2], W, H, 51), "qp 51")


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_stage_pointers_off_16(torch_cuda, contexts, offset):
    """d_first, d_first4 and d_out 4, 8, 12 bytes behind a 16-byte boundary, alone and together: the same bytes (8 leaves the inputs' wide path, 4 and 12 do not)"""
    size = ip.DRAW_SIZES[0]
    ctx, d = contexts[size], ip.draw(size)
    for kw in (dict(in_offset=offset), dict(in4_offset=offset), dict(out_offset=offset), dict(in_offset=offset, in4_offset=16 - offset, out_offset=offset)):
        ip.same(run_stage(torch_cuda, ctx, d["first"], d["first4"], ip.DRAW_QP, **kw), d["out"], kw)
    ip.same(run_stage(torch_cuda, ctx, d["first"], None, ip.DRAW_QP, in_offset=offset, out_offset=16 - offset), d["out_no4"], "no 4x4 records")


def test_stage_more_ctus_than_the_grid(torch_cuda, contexts):
    """8 400 CTUs: the draw of 200 x 136 tiled 50 times (700 pictures of 12 CTUs); the grid holds at most 8 workgroups of four CTUs per CU"""
    size = ip.DRAW_SIZES[0]
    ctx, d = contexts[size], ip.draw(size)
    reps = 50
    first, first4 = np.tile(d["first"], (reps, 1, 1)), np.tile(d["first4"], (reps, 1, 1))
    assert first.shape[0] * first.shape[1] == 8400
    got = run_stage(torch_cuda, ctx, first, first4, ip.DRAW_QP, out_offset=4)
    exp = np.tile(d["out"], (reps, 1, 1))
    assert got.tobytes() == exp.tobytes()


def test_stage_two_streams_with_different_qps(torch_cuda, contexts):
    size = ip.DRAW_SIZES[0]
    ctx, d = contexts[size], ip.draw(size)
    W, H = size
    qps = (22, 47)
    exp = [ip.stage(d["first"], d["first4"], W, H, qp) for qp in qps]
    assert exp[0].tobytes() != exp[1].tobytes()
    held, held4 = to_dev(torch_cuda, d["first"]), to_dev(torch_cuda, d["first4"])
    streams = [torch_cuda.cuda.Stream() for _ in qps]
    outs = [[Guarded(torch_cuda, d["first"].size * 16) for _ in range(3)] for _ in qps]
    torch_cuda.cuda.synchronize()
    for r in range(3):
        for s, qp, o in zip(streams, qps, outs):
            ctx.intra_p_device(P, held.data_ptr(), held4.data_ptr(), o[r].ptr, stream=s.cuda_stream, qp=qp)
    torch_cuda.cuda.synchronize()
    for e, o in zip(exp, outs):
        for r in range(3):
            ip.same(o[r].result(IDT, e.shape), e, r)


# ---- 2. real records: first pass -> 4x4 first pass -> stage on one stream ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bd, dtype", [(8, np.uint8), (8, np.int16), (10, np.int16), (12, np.int16)])
def test_stage_on_real_records_of_one_stream(torch_cuda, bd, dtype):
    from oracle import oracle_py as op
    oracle = op.load_oracle()
    W, H, qp = 100, 76, 27
    rng = np.random.default_rng(90 + bd)
    yy, xx = np.mgrid[0:H, 0:W]
    pic = np.clip((xx * 3 + yy * 2) % 256 + rng.integers(-20, 21, size=(H, W)), 0, 255).astype(np.int64) << (bd - 8)
    pic[:40, :48] = 1 << (bd - 1)                                   # a flat corner: planar at SATD 0
    if bd > 8:
        pic = np.clip(pic + rng.integers(0, 1 << (bd - 8), size=(H, W)), 0, (1 << bd) - 1)
    first, first4 = ip.oracle_first_passes(oracle, op, pic, bd, qp)
    exp = ip.stage(first[None], first4[None], W, H, qp)
    assert (exp["part"] == 1).any() and (exp["part"][exp["cost_best"] != ip.MARK] == 0).any() and (exp["cost_best"] == ip.MARK).any()
    ctx = capi.Context(W, H, bd)
    item = np.dtype(dtype).itemsize
    buf, org, stride = pel(pic)
    planes = to_dev(torch_cuda, buf.astype(dtype))
    n = ctx.num_ctus
    d_first, d_first4, out = Guarded(torch_cuda, n * 85 * 16), Guarded(torch_cuda, n * 256 * 16), Guarded(torch_cuda, n * 85 * 16)
    stream = torch_cuda.cuda.Stream()
    torch_cuda.cuda.synchronize()
    ptr = planes.data_ptr() + item * org
    ctx.intra_first_pass_device(ptr, item, stride, 0, 1, d_first.ptr, stream=stream.cuda_stream, qp=qp)
    ctx.intra_first_pass_4x4_device(ptr, item, stride, 0, 1, d_first4.ptr, None, stream=stream.cuda_stream, qp=qp)
    ctx.intra_p_device(1, d_first.ptr, d_first4.ptr, out.ptr, stream=stream.cuda_stream, qp=qp)
    torch_cuda.cuda.synchronize()
    g_first, g_first4 = d_first.result(NDT, (n, 85)), d_first4.result(NDT, (n, 256))
    assert np.array_equal(g_first["satd"], first["satd"]) and np.array_equal(g_first["mode"], first["mode"])
    assert np.array_equal(g_first4["satd"], first4["satd"]) and np.array_equal(g_first4["mode"], first4["mode"])
    ip.same(out.result(IDT, (1, n, 85)), exp, (bd, dtype.__name__))
    # the host form on the same records
    ip.same(ctx.intra_p(first, first4, qp=qp)[None], exp, "host form")
    ip.same(ctx.intra_p(first, None, qp=qp)[None], ip.stage(first[None], None, W, H, qp), "host form, no 4x4 records")
    ctx.close()


# ---- 3. the tree kernel on the draw -------------------------------------------------------------------------------------------------------------------------

def run_tree(torch, ctx, shapes, merge, skip, mask, intra, rule, rows=None, want=ALL, offsets=(0, 0, 0, 0), map_offset=0, tree_offset=0, skip_only=False):
    """one call, then a synchronise -> (records, depth_min, depth_max), None for an output not asked for; guards checked, and an output that was not asked for
    stays untouched.  skip_only: fhevc_p_tree_select_skip_device on the same records"""
    n_p, nb = shapes.shape[:2]
    held = [at_offset(torch, a, o) for a, o in zip((shapes, merge, skip, intra), offsets)]
    dmin, dmax, tree = Guarded(torch, n_p * nb * 256, map_offset), Guarded(torch, n_p * nb * 256, map_offset), Guarded(torch, n_p * nb * 85 * 16, tree_offset)
    torch.cuda.synchronize()
    outs = (dmin.ptr if want[0] else None, dmax.ptr if want[1] else None, tree.ptr if want[2] else None)
    if skip_only:
        ctx.p_tree_select_skip_device(held[0][1], held[1][1], held[2][1], mask, n_p, *outs, rows=rows, rule=rule)
    else:
        ctx.p_tree_select_intra_device(held[0][1], held[1][1], held[2][1], mask, held[3][1], n_p, *outs, rows=rows, rule=rule)
    torch.cuda.synchronize()
    for g, w in zip((dmin, dmax, tree), want):
        assert w or g.untouched()
    return (tree.result(TDT, (n_p, nb, 85)) if want[2] else None, dmin.result(np.uint8, (n_p, nb, 256)) if want[0] else None,
            dmax.result(np.uint8, (n_p, nb, 256)) if want[1] else None)


def same_all(got, exp, what):
    if got[0] is not None:
        ip.same_tree(got[0], exp[0], what)
    for i, n in ((1, "depth_min"), (2, "depth_max")):
        if got[i] is not None:
            assert np.array_equal(got[i], exp[i]), (what, n, np.argwhere(got[i] != exp[i])[:5])


@pytest.mark.parametrize("size", ip.DRAW_SIZES)
def test_tree_on_the_draw_four_rules_and_every_mask(torch_cuda, contexts, size):
    W, H = size
    ctx, d = contexts[size], ip.draw(size)
    cw, ch = (W + 63) // 64, (H + 63) // 64
    ins = (d["shapes"], d["merge"], d["skip"])
    for rname, mask in itertools.product(d["rules"], range(4)):
        same_all(run_tree(torch_cuda, ctx, *ins, mask, d["intra"], d["rules"][rname]), ip.draw_tree(size, rname, mask), (rname, mask))
    assert (ip.draw_tree(size, "r1", 3)[0]["pad"][..., 0] == 1).any()
    # every combination of NULL outputs
    for want in itertools.product((True, False), repeat=3):
        if any(want) and want != ALL:
            same_all(run_tree(torch_cuda, ctx, *ins, 3, d["intra"], d["rules"]["r2"], want=want), ip.draw_tree(size, "r2", 3), want)
    same_all(run_tree(torch_cuda, ctx, *ins, 1, d["intra"], None), ip.draw_tree(size, "default", 1), "rule NULL")
    # bands
    for rows in ((1, 2), (0, 1), (1, ch)):
        got = run_tree(torch_cuda, ctx, *(band(a, rows, cw) for a in ins), 2, band(d["intra"], rows, cw), d["rules"]["r3"], rows=rows)
        same_all(got, tuple(band(e, rows, cw) for e in ip.draw_tree(size, "r3", 2)), rows)
    # all-MARK intra records: byte for byte the tree that stops at a skip
    blank = ip.all_mark(d["intra"])
    for rname, mask in (("default", 3), ("r2", 0), ("r1", 1)):
        a = run_tree(torch_cuda, ctx, *ins, mask, blank, d["rules"][rname])
        b = run_tree(torch_cuda, ctx, *ins, mask, blank, d["rules"][rname], skip_only=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (rname, mask)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_tree_pointers_off_their_alignment(torch_cuda, contexts, offset):
    """d_shapes, d_merge, d_skip, d_intra and d_tree 4, 8, 12 bytes behind a 16-byte boundary, the maps 1, 2, 3 bytes: the same bytes"""
    size = ip.DRAW_SIZES[0]
    ctx, d = contexts[size], ip.draw(size)
    ins = (d["shapes"], d["merge"], d["skip"])
    exp = ip.draw_tree(size, "r1", 3)
    for kw in (dict(offsets=(4 * offset, 0, 0, 0)), dict(offsets=(0, 4 * offset, 0, 0)), dict(offsets=(0, 0, 4 * offset, 0)), dict(offsets=(0, 0, 0, 4 * offset)),
               dict(tree_offset=4 * offset), dict(map_offset=offset),
               dict(offsets=(4 * offset, 16 - 4 * offset, 4 * offset, 16 - 4 * offset), tree_offset=16 - 4 * offset, map_offset=offset)):
        same_all(run_tree(torch_cuda, ctx, *ins, 3, d["intra"], d["rules"]["r1"], **kw), exp, kw)


def test_tree_more_ctus_than_the_grid(torch_cuda, contexts):
    size = ip.DRAW_SIZES[0]
    ctx, d = contexts[size], ip.draw(size)
    reps = 50
    tiled = [np.tile(d[n], (reps, 1, 1)) for n in ("shapes", "merge", "skip", "intra")]
    got = run_tree(torch_cuda, ctx, tiled[0], tiled[1], tiled[2], 3, tiled[3], d["rules"]["r2"])
    for g, e in zip(got, ip.draw_tree(size, "r2", 3)):
        assert g.tobytes() == np.tile(e, (reps, 1, 1)).tobytes()


# ---- 4. the frame chain ---------------------------------------------------------------------------------------------------------------------------------------

def frame_pieces(torch, ctx, cur, ref, bd, qp, search_range, coarse_range, mask, shapes, merge):
    """what the chain must give behind its selection, from the device forms of its pieces run one by one on the records the chain downloaded:
    the skip stage at the chain's merge range, the two first passes of the current picture, the intra stage, the tree -> (intra, records, depth_min, depth_max)"""
    n = ctx.num_ctus
    planes, org, stride, fstride = pel_batch([ref, cur])
    d_planes = to_dev(torch, planes)
    ptr = d_planes.data_ptr() + 2 * org
    d_merge, d_shapes = to_dev(torch, merge), to_dev(torch, shapes)
    g = {k: Guarded(torch, size) for k, size in (("skip", n * 85 * 16), ("first", n * 85 * 16), ("first4", n * 256 * 16), ("intra", n * 85 * 16), ("tree", n * 85 * 16),
                                                 ("dmin", n * 256), ("dmax", n * 256))}
    torch.cuda.synchronize()
    merge_range = 64 if coarse_range else search_range
    ctx.motion_skip_device(ptr, 2, stride, fstride, 2, d_merge.data_ptr(), g["skip"].ptr, qp=qp, max_range=merge_range)
    cur_ptr = ptr + 2 * fstride
    ctx.intra_first_pass_device(cur_ptr, 2, stride, 0, 1, g["first"].ptr, qp=qp)
    ctx.intra_first_pass_4x4_device(cur_ptr, 2, stride, 0, 1, g["first4"].ptr, None, qp=qp)
    ctx.intra_p_device(1, g["first"].ptr, g["first4"].ptr, g["intra"].ptr, qp=qp)
    ctx.p_tree_select_intra_device(d_shapes.data_ptr(), d_merge.data_ptr(), g["skip"].ptr, mask, g["intra"].ptr, 1, g["dmin"].ptr, g["dmax"].ptr, g["tree"].ptr)
    torch.cuda.synchronize()
    return (g["intra"].result(IDT, (n, 85)), g["tree"].result(TDT, (n, 85)), g["dmin"].result(np.uint8, (n, 256)), g["dmax"].result(np.uint8, (n, 256)),
            g["skip"].result(capi.MOTION_SKIP_DTYPE, (n, 85)))


@pytest.mark.parametrize("bd", [8, 10])
def test_the_constructed_pair_through_the_whole_chain(torch_cuda, bd):
    """128 x 64 at qp 32 (tests/test_intra_p_ref.py confirms the intra side on the CPU): CTU 0 is flat -- every intra record satd 0, mode 0, cost c[2]; the
    root's cost_tree == c[2] with the intra bit; both maps 0 everywhere.  CTU 1 is the reference displaced by half a sample: no node carries the intra bit,
    and its maps are what the tree that stops at a skip gives."""
    from oracle import oracle_py as op
    cur, ref = ip.constructed_pair(bd)
    W, H, qp = ip.PAIR_W, ip.PAIR_H, ip.PAIR_QP
    c2 = ip.bit_costs(qp)[2]
    ctx = capi.Context(W, H, bd)
    (cbuf, org, stride), (rbuf, _, _) = pel(cur), pel(ref)
    dmin, dmax, shapes, merge, intra = ctx.p_tree_intra_frame(cbuf, rbuf, origin=org, stride=stride, qp=qp, search_range=8, skip_mask=3, with_shapes=True,
                                                              with_merge=True, with_intra=True)
    first, first4 = ip.oracle_first_passes(op.load_oracle(), op, cur, bd, qp)
    ip.same(intra[None], ip.stage(first[None], first4[None], W, H, qp), "the chain's intra records against oracle + restatement")
    assert (intra["satd_best"][0] == 0).all() and (intra["cost_best"][0] == c2).all() and (intra["modes"][0] == 0).all() and (intra["part"][0] == 0).all()
    p_intra, rec, pmin, pmax, skip = frame_pieces(torch_cuda, ctx, cur, ref, bd, qp, 8, 0, 3, shapes, merge)
    assert p_intra.tobytes() == intra.tobytes() and np.array_equal(pmin, dmin) and np.array_equal(pmax, dmax)
    # every download and every piece against the CPU restatement of the whole chain (tests/test_intra_p_ref.py confirms the statements on it)
    g = ip.constructed_chain(op.load_oracle(), op, bd)
    assert shapes.tobytes() == g["shapes"].tobytes() and merge.tobytes() == g["merge"].tobytes() and skip.tobytes() == g["skip"].tobytes()
    ip.same(intra[None], g["intra"][None], "intra records against the chain restatement")
    ip.same_tree(rec[None], g["tree"][None], "tree records against the chain restatement")
    assert np.array_equal(dmin, g["dmin"]) and np.array_equal(dmax, g["dmax"])
    ip.check_constructed(dict(intra=intra, tree=rec, dmin=dmin, dmax=dmax, skip_dmin=g["skip_dmin"], skip_dmax=g["skip_dmax"]), c2)
    # the tree records are the restatement's on the chain's own records
    erec, emin, emax = ip.tree_select(shapes[None], merge[None], skip[None], 3, intra[None], W, H)
    ip.same_tree(rec[None], erec, "tree")
    assert np.array_equal(dmin[None], emin) and np.array_equal(dmax[None], emax)
    # CTU 0
    assert int(rec["cost_tree"][0, 0]) == c2 and rec["pad"][0, 0, 0] == 1 and (rec["pad"][0, :, 0] == 1).all()
    assert not dmin[0].any() and not dmax[0].any()
    assert min(int(shapes["cost_best"][0].min()), int(merge["cost_best"][0].min())) > c2, "a flat CTU against noise: every inter cost lies above c[2]"
    # CTU 1
    assert not rec["pad"][1].any()
    smin, smax = capi.p_tree_select_skip(shapes, merge, skip, 3, W, H)
    assert np.array_equal(dmin[1], smin[1]) and np.array_equal(dmax[1], smax[1])
    ctx.close()


@pytest.mark.parametrize("coarse_range", [0, 4])
def test_frame_against_its_pieces_and_its_counters(torch_cuda, coarse_range):
    W, H, qp, bd = 200, 136, 30, 8
    rng = np.random.default_rng(55)
    ref = rng.integers(0, 256, size=(H, W)).astype(np.int64)
    cur = np.roll(ref, (1, -2), axis=(0, 1))
    cur[:64, :64] = 128                                                 # a flat CTU in the corner, a flat 16x16 and an 8x8 block of new content
    cur[80:96, 16:32] = 60
    cur[72:80, 136:144] = 200
    ctx = capi.Context(W, H, bd)
    n = ctx.num_ctus
    (cbuf, org, stride), (rbuf, _, _) = pel(cur), pel(ref)
    kw = dict(origin=org, stride=stride, qp=qp, search_range=8, coarse_range=coarse_range)
    a_min, a_max, a_shapes, a_merge = ctx.p_tree_amvp_frame(cbuf, rbuf, with_shapes=True, with_merge=True, **kw)
    s0 = ctx.stats()
    ctx.p_tree_amvp_frame(cbuf, rbuf, with_shapes=True, with_merge=True, **kw)
    s1 = ctx.stats()
    from oracle import oracle_py as op
    whole = {m: ip.chain(op.load_oracle(), op, cur, ref, bd, qp, m) for m in (3, 0)} if coarse_range == 0 else {}
    for mask in (3, 0):
        before = ctx.stats()
        dmin, dmax, shapes, merge, intra = ctx.p_tree_intra_frame(cbuf, rbuf, skip_mask=mask, with_shapes=True, with_merge=True, with_intra=True, **kw)
        after = ctx.stats()
        assert shapes.tobytes() == a_shapes.tobytes() and merge.tobytes() == a_merge.tobytes(), "the stages before the skip stage are fhevc_p_tree_amvp_frame's"
        assert after["bytes_h2d"] - before["bytes_h2d"] == W * H * 4
        assert after["bytes_d2h"] - before["bytes_d2h"] == n * (2 * 256 + 3 * 85 * 16)
        # the skip stage, two first passes and the intra stage more than the chain without them
        assert after["kernels_launched"] - before["kernels_launched"] == s1["kernels_launched"] - s0["kernels_launched"] + 4
        p_intra, rec, pmin, pmax, skip = frame_pieces(torch_cuda, ctx, cur, ref, bd, qp, 8, coarse_range, mask, shapes, merge)
        assert p_intra.tobytes() == intra.tobytes() and np.array_equal(pmin, dmin) and np.array_equal(pmax, dmax), mask
        erec, emin, emax = ip.tree_select(shapes[None], merge[None], skip[None], mask, intra[None], W, H)
        ip.same_tree(rec[None], erec, mask)
        assert np.array_equal(dmin[None], emin) and np.array_equal(dmax[None], emax)
        assert rec["pad"][0, 0, 0] == 1 and not dmax[0].any(), "the flat CTU is one intra CU"
        if mask in whole:     # the zero-centred chain against the CPU restatement of the whole chain
            g = whole[mask]
            assert shapes.tobytes() == g["shapes"].tobytes() and merge.tobytes() == g["merge"].tobytes() and skip.tobytes() == g["skip"].tobytes()
            ip.same(intra[None], g["intra"][None], mask)
            ip.same_tree(rec[None], g["tree"][None], mask)
            assert np.array_equal(dmin, g["dmin"]) and np.array_equal(dmax, g["dmax"])
    # without the optional downloads only the maps come back
    before = ctx.stats()
    m2 = ctx.p_tree_intra_frame(cbuf, rbuf, skip_mask=0, **kw)
    assert ctx.stats()["bytes_d2h"] - before["bytes_d2h"] == n * 512 and np.array_equal(m2[0], dmin) and np.array_equal(m2[1], dmax)
    # rejected: nothing moves
    before = ctx.stats()
    out = np.full(n * 256, CANARY, np.uint8)
    cp, rp = cbuf.reshape(-1).ctypes.data + 2 * org, rbuf.reshape(-1).ctypes.data + 2 * org
    o = out.ctypes.data
    for args in ((cp, rp, stride, qp, 8, coarse_range, None, None, 4, o, o, None, None, None), (cp, rp, stride, qp, 8, coarse_range, None, None, -1, o, o, None, None, None),
                 (cp, rp, stride, 52, 8, coarse_range, None, None, 3, o, o, None, None, None), (None, rp, stride, qp, 8, coarse_range, None, None, 3, o, o, None, None, None),
                 (cp, rp, stride, qp, 8, coarse_range, None, None, 3, None, o, None, None, None), (cp, rp, W - 1, qp, 8, coarse_range, None, None, 3, o, o, None, None, None),
                 (cp, rp, stride, qp, 0, coarse_range, None, None, 3, o, o, None, None, None), (cp, rp, stride, qp, 8, 15, None, None, 3, o, o, None, None, None)):
        assert ctx.lib.fhevc_p_tree_intra_frame(ctx.h, *args) == capi.E_INVALID, args
    assert ctx.stats() == before and (out == CANARY).all()
    ctx.close()


# ---- 5. rejected calls and the timing slots -----------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_and_the_timing_slots(torch_cuda, contexts):
    size = ip.DRAW_SIZES[0]
    ctx, d = contexts[size], ip.draw(size)
    ch = 3
    ctx.enable_kernel_timing(True)
    slots = (17, 19, 21, 23, 25, 27)
    for s in slots:
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls in (1, 2, 3):
        run_stage(torch_cuda, ctx, d["first"], d["first4"] if calls != 2 else None, ip.DRAW_QP)
        ms, count = ctx.kernel_timing(27)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (17, 19, 21, 23, 25))
    run_tree(torch_cuda, ctx, d["shapes"], d["merge"], d["skip"], 3, d["intra"], None)
    assert ctx.kernel_timing(17)[1] == 1 and ctx.kernel_timing(27)[1] == 3
    ctx.enable_kernel_timing(False)
    for s in (26, 28):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
    held, out = to_dev(torch_cuda, d["first"]), Guarded(torch_cuda, d["first"].size * 16)
    launched = ctx.stats()["kernels_launched"]
    lib, h, p, o = ctx.lib, ctx.h, held.data_ptr(), out.ptr
    for args in ((None, 1, 0, ch, 32, p, None, o, None), (h, 1, 0, ch, 32, None, None, o, None), (h, 1, 0, ch, 32, p, None, None, None), (h, 1, 0, ch, 32, p + 2, None, o, None),
                 (h, 1, 0, ch, 32, p, p + 1, o, None), (h, 1, 0, ch, 32, p, None, o + 2, None), (h, 0, 0, ch, 32, p, None, o, None), (h, -1, 0, ch, 32, p, None, o, None),
                 (h, 1, -1, ch, 32, p, None, o, None), (h, 1, 0, ch + 1, 32, p, None, o, None), (h, 1, 2, 1, 32, p, None, o, None), (h, 1, 0, ch, -1, p, None, o, None),
                 (h, 1, 0, ch, 52, p, None, o, None)):
        if args[0] is not None:      # leave another call's text behind, so that a rejection that writes none would show
            assert lib.fhevc_kernel_timing(h, 0, 0, None, None) == capi.OK and lib.fhevc_p_tree_select_intra_device(h, p, p, p, 9, p, 1, 0, ch, None, o, None, None, None) == capi.E_INVALID
            assert b"skip_mask" in lib.fhevc_last_error(h)
        assert lib.fhevc_intra_p_device(*args) == capi.E_INVALID, args
        if args[0] is not None:
            text = lib.fhevc_last_error(h)
            assert b"skip_mask" not in text and any(t in text for t in (b"intra-stage", b"frame layout", b"CTU-row band", b"qp out of range")), (args, text)
    # the tree: what fhevc_p_tree_select_skip_device rejects, a null intra pointer, a record pointer off its 4-byte alignment
    for args in ((h, p, p, p, 3, None, 1, 0, ch, None, o, None, None, None), (h, p, p, None, 3, p, 1, 0, ch, None, o, None, None, None),
                 (h, p, None, p, 3, p, 1, 0, ch, None, o, None, None, None), (h, None, p, p, 3, p, 1, 0, ch, None, o, None, None, None),
                 (h, p, p, p, 4, p, 1, 0, ch, None, o, None, None, None), (h, p, p, p, 3, p, 0, 0, ch, None, o, None, None, None),
                 (h, p, p, p, 3, p + 2, 1, 0, ch, None, o, None, None, None), (h, p + 1, p, p, 3, p, 1, 0, ch, None, o, None, None, None),
                 (h, p, p, p + 3, 3, p, 1, 0, ch, None, None, None, o + 2, None),
                 (h, p, p, p, 3, p, 1, 0, ch, None, None, None, None, None), (h, p, p, p, 3, p, 1, 0, ch + 1, None, o, None, None, None),
                 (h, p, p, p, 3, p, 1, 0, ch, C.byref(capi.p_tree_rule(stop_q8=[0, 65536, 0])), o, None, None, None)):
        assert lib.fhevc_p_tree_select_intra_device(*args) == capi.E_INVALID, args
    # the host form
    first = np.ascontiguousarray(d["first"][0])
    res = np.full(first.size * 16, CANARY, np.uint8)
    moved = ctx.stats()
    for args in ((h, 52, first.ctypes.data, None, res.ctypes.data), (h, -1, first.ctypes.data, None, res.ctypes.data), (h, 32, None, None, res.ctypes.data),
                 (h, 32, first.ctypes.data, None, None)):
        assert lib.fhevc_intra_p(*args) == capi.E_INVALID, args
    torch_cuda.cuda.synchronize()
    assert out.untouched() and (res == CANARY).all() and ctx.stats() == moved and moved["kernels_launched"] == launched
