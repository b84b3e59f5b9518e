"""The partition-size selection on the device: fhevc_pu_shape_select_device (k_pu_shape.hip) and fhevc_p_shape_frame, bit for bit -- every field of
every record and every cost, nothing sampled.  Expected values come from the numpy restatement tests/pu_shape_ref.py (pinned to hand-computed cases
by tests/test_pu_shape_ref.py) and are cross-checked against the library's host function; nothing is compared with the kernel's own output except
where two launches must give the same bytes (unaligned inputs, repeated pictures).

The selection needs no planes: its context is 200 x 136 = 4 x 3 CTUs, ragged on both sides by 8 samples, so the last column and row hold
edge-crossing nodes of all levels."""
import ctypes as C

import numpy as np
import pytest

import motion_refine_ref as mr
import pu_shape_cases as pc
import pu_shape_ref as sr
from fasthevc_amd import capi
from motion_gpu_helpers import CANARY, clip_planes, pel_batch, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

W, H = 200, 136
CW, CH = 4, 3
N = CW * CH
QDT, SDT = capi.MOTION_QPEL_DTYPE, capi.SHAPE_DTYPE
_CACHE = {}


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


def random_case():
    """2 pictures of 12 CTUs of random entries, three rules, and their expected records and costs (with and without the small PUs); computed once"""
    if "random" not in _CACHE:
        rng = np.random.default_rng(811)
        ins = sr.random_entries(rng, 2, N)
        rules = {"default": capi.pu_shape_rule_default(), "amp0": sr.random_rule(rng, 0), "amp1": sr.random_rule(rng, 1)}
        exp = {name: sr.select(*ins, W, H, rule=r) for name, r in rules.items()}
        exp_no_small = sr.select(ins[0], ins[1], None, W, H, rule=rules["amp1"])
        _CACHE["random"] = (ins, rules, exp, exp_no_small)
    return _CACHE["random"]


def band(a, rows):
    return np.ascontiguousarray(a[:, rows[0] * CW:rows[1] * CW])


def run(torch, ctx, ins, rule, rows=(0, CH), want_costs=True, use_small=True, in_offset=0, out_offset=0, stream=None):
    """one call, then a synchronise -> (records [P, band CTUs, 85], costs [P, band CTUs, 85, 8] or None); guards checked"""
    P, nb = ins[0].shape[:2]
    held = [at_offset(torch, a, in_offset) for a in ins]
    shapes, costs = Guarded(torch, P * nb * 85 * 16, out_offset), Guarded(torch, P * nb * 85 * 32, out_offset)
    torch.cuda.synchronize()
    ctx.pu_shape_select_device(held[0][1], held[1][1], held[2][1] if use_small else None, P, shapes.ptr, costs.ptr if want_costs else None, rows=rows,
                               stream=stream, rule=rule)
    torch.cuda.synchronize()
    if not want_costs:
        assert costs.untouched()
    return shapes.result(SDT, (P, nb, 85)), costs.result(np.uint32, (P, nb, 85, 8)) if want_costs else None


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    c = capi.Context(W, H, 8)
    assert (c.ctus_x, c.ctus_y) == (CW, CH)
    yield c
    c.close()


# ---- 1. random inputs: the restatement, the host function, the kernel -------------------------------------------------------------------------------

def test_random_inputs_equal_the_restatement_and_the_host_function(torch_cuda, ctx):
    ins, rules, exp, exp_no_small = random_case()
    # the draw reaches the edge cases, and the edge of the picture invalidates nodes of every level
    rec, costs = exp["amp1"]
    assert (costs == sr.SATURATED).any() and ((rec["best"] != 255) & (rec["cost_best"] == rec["cost_second"])).any()
    assert ((rec["mask"] != 0) & (rec["cost_2Nx2N"] == sr.MARKER)).any() and (rec["avail"] & ~rec["mask"] & 0xF0 != 0).any()
    assert {sr.level(k) for k in np.flatnonzero(rec["mask"][0, CW - 1] == 0)} == {0, 1, 2, 3}
    assert {sr.level(k) for k in np.flatnonzero(rec["mask"][0, N - CW] == 0)} == {0, 1, 2, 3}
    for name, rule in rules.items():
        erec, ecosts = exp[name]
        for p in range(2):
            hrec, hcosts = capi.pu_shape_select(ins[0][p], ins[1][p], ins[2][p], W, H, rule, with_costs=True)
            sr.same(hrec, erec[p], ("host", name, p))
            assert np.array_equal(hcosts, ecosts[p]), ("host", name, p)
        grec, gcosts = run(torch_cuda, ctx, ins, rule)
        sr.same(grec, erec, ("device", name))
        assert np.array_equal(gcosts, ecosts), ("device", name, np.argwhere(gcosts != ecosts)[:5])
        nrec, _ = run(torch_cuda, ctx, ins, rule, want_costs=False)
        sr.same(nrec, erec, ("device without d_costs", name))
    grec, gcosts = run(torch_cuda, ctx, ins, rules["amp1"], use_small=False)
    sr.same(grec, exp_no_small[0], "device without d_pus_small")
    assert np.array_equal(gcosts, exp_no_small[1]) and not np.array_equal(gcosts, exp["amp1"][1])
    # rule NULL is the documented default
    drec, _ = run(torch_cuda, ctx, ins, None)
    sr.same(drec, exp["default"][0], "rule NULL")


# ---- 2. unaligned pointers give the same bytes (entries are read as dwords at any alignment; unaligned outputs take the dword-store instantiation) ------------

@pytest.mark.parametrize("offset", [4, 8, 12])
def test_unaligned_inputs_give_the_same_bytes(torch_cuda, ctx, offset):
    ins, rules, exp, _ = random_case()
    arec, acosts = run(torch_cuda, ctx, ins, rules["amp0"])
    sr.same(arec, exp["amp0"][0], "aligned")
    grec, gcosts = run(torch_cuda, ctx, ins, rules["amp0"], in_offset=offset)
    assert grec.tobytes() == arec.tobytes() and gcosts.tobytes() == acosts.tobytes()
    # ... and with the outputs off the 16-byte grid as well (entries and records are 4-byte aligned by type)
    grec, gcosts = run(torch_cuda, ctx, ins, rules["amp0"], in_offset=offset, out_offset=16 - offset)
    assert grec.tobytes() == arec.tobytes() and gcosts.tobytes() == acosts.tobytes()


# ---- 3. bands and extents ------------------------------------------------------------------------------------------------------------------------------

def test_bands_and_extents(torch_cuda, ctx):
    torch = torch_cuda
    ins, rules, exp, _ = random_case()
    erec, ecosts = exp["amp1"]
    for rows in ((0, CH), (1, 2), (1, 3)):          # the guards are checked inside run()
        bins = tuple(band(a, rows) for a in ins)
        brec, bcosts = run(torch, ctx, bins, rules["amp1"], rows=rows)
        # a band's CTUs keep their place in the picture: the expected values of the band are the band of the expected values
        xrec, xcosts = sr.select(*bins, W, H, rows=rows, rule=rules["amp1"])
        sr.same(xrec, band(erec, rows), rows)
        sr.same(brec, xrec, rows)
        assert np.array_equal(bcosts, xcosts), rows
    # an empty band writes nothing and launches nothing
    held = [to_dev(torch, a) for a in ins]
    shapes, costs = Guarded(torch, 4096), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.pu_shape_select_device(held[0].data_ptr(), held[1].data_ptr(), held[2].data_ptr(), 2, shapes.ptr, costs.ptr, rows=(2, 2))
    torch.cuda.synchronize()
    assert shapes.untouched() and costs.untouched() and ctx.stats()["kernels_launched"] == launched


def test_more_ctus_than_the_persistent_grid(torch_cuda, ctx):
    """700 pictures that repeat the two random ones = 8 400 CTUs in one launch, more than the grid's cap of eight workgroups of four waves on each of 256
    CUs: every repeat equals the first two pictures, and those equal the restatement"""
    ins, rules, exp, _ = random_case()
    P = 700
    assert P * N > 8 * 4 * 256
    big = tuple(np.tile(a, (P // 2, 1, 1)) for a in ins)
    grec, gcosts = run(torch_cuda, ctx, big, rules["amp1"])
    sr.same(grec[:2], exp["amp1"][0], "first pictures")
    assert np.array_equal(gcosts[:2], exp["amp1"][1])
    first_r, first_c = grec[:2].tobytes(), gcosts[:2].tobytes()
    for p in range(2, P, 2):
        assert grec[p:p + 2].tobytes() == first_r and gcosts[p:p + 2].tobytes() == first_c, p


# ---- 4. the rule is per call: two streams -----------------------------------------------------------------------------------------------------------------

def test_two_rules_in_flight_on_two_streams(torch_cuda, ctx):
    torch = torch_cuda
    ins, rules, exp, _ = random_case()
    assert not np.array_equal(exp["amp0"][0]["mask"], exp["amp1"][0]["mask"])
    held = [to_dev(torch, a) for a in ins]
    outs = [(Guarded(torch, 2 * N * 85 * 16), Guarded(torch, 2 * N * 85 * 32)) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    scratch = capi.PuShapeRule()
    for name, s, (shapes, costs) in (("amp0", streams[0], outs[0]), ("amp1", streams[1], outs[1])):
        C.memmove(C.byref(scratch), C.byref(rules[name]), C.sizeof(scratch))
        ctx.pu_shape_select_device(held[0].data_ptr(), held[1].data_ptr(), held[2].data_ptr(), 2, shapes.ptr, costs.ptr, stream=s.cuda_stream, rule=scratch)
        C.memset(C.byref(scratch), 0, C.sizeof(scratch))      # the rule was read during the call
    torch.cuda.synchronize()
    for name, (shapes, costs) in zip(("amp0", "amp1"), outs):
        sr.same(shapes.result(SDT, (2, N, 85)), exp[name][0], name)
        assert np.array_equal(costs.result(np.uint32, (2, N, 85, 8)), exp[name][1]), name


# ---- 5. the real pipeline on one stream, no host synchronisation ----------------------------------------------------------------------------------------------

def pipeline(torch, bd):
    """search, refinement and three selections (default rule, the wide margin with and without the AMP gate) queued on one stream ->
    dict(refined: {family: [numCtus, per]}, rec / costs per rule name, ctx geometry); computed once per bit depth"""
    if ("pipe", bd) not in _CACHE:
        cur, ref = pc.pictures()
        pics = clip_planes([ref, cur], bd, low_bits_seed=7)
        if bd > 8:
            assert any((p & ((1 << (bd - 8)) - 1)).any() for p in pics)
        flat, org, stride, fs = pel_batch(pics)
        c = capi.Context(pc.W, pc.H, bd)
        n = c.num_ctus
        d_luma = to_dev(torch, flat)
        per = (85, 124, 384)
        found = [Guarded(torch, n * k * 16) for k in per]
        refined = [Guarded(torch, n * k * 16) for k in per]
        names = ("default", "amp1", "amp0")
        outs = {name: (Guarded(torch, n * 85 * 16), Guarded(torch, n * 85 * 32)) for name in names}
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ptr = d_luma.data_ptr() + 2 * org
        c.motion_search_pu_wide_device(ptr, 2, stride, fs, 2, found[0].ptr, found[1].ptr, found[2].ptr, stream=s.cuda_stream, qp=pc.QP, search_range=pc.RANGE)
        c.motion_refine_pu_wide_device(ptr, 2, stride, fs, 2, found[0].ptr, refined[0].ptr, found[1].ptr, refined[1].ptr, found[2].ptr, refined[2].ptr,
                                       stream=s.cuda_stream, qp=pc.QP, max_range=pc.RANGE)
        for name, rule in zip(names, pc.rules()):
            c.pu_shape_select_device(refined[0].ptr, refined[1].ptr, refined[2].ptr, 1, outs[name][0].ptr, outs[name][1].ptr, stream=s.cuda_stream, rule=rule)
        torch.cuda.synchronize()
        res = dict(refined=[g.result(QDT, (1, n, k)) for g, k in zip(refined, per)], planes=(flat, org, stride), n=n)
        for name in names:
            res[name] = (outs[name][0].result(SDT, (n, 85)), outs[name][1].result(np.uint32, (n, 85, 8)))
        c.close()
        _CACHE[("pipe", bd)] = res
    return _CACHE[("pipe", bd)]


@pytest.mark.parametrize("bd", [8, 10])
def test_search_refinement_and_selection_on_one_stream(oracle, torch_cuda, bd):
    res = pipeline(torch_cuda, bd)
    refined = res["refined"]
    assert (refined[1]["cost_best"] != sr.MARKER).any() and (refined[0]["mvx"] != 0).any()
    for name, rule in zip(("default", "amp1", "amp0"), pc.rules()):
        erec, ecosts = sr.select(*refined, pc.W, pc.H, rule=rule)
        sr.same(res[name][0], erec[0], (bd, name))
        assert np.array_equal(res[name][1], ecosts[0]), (bd, name)
        hrec = capi.pu_shape_select(refined[0][0], refined[1][0], refined[2][0], pc.W, pc.H, rule)
        sr.same(hrec, erec[0], (bd, name, "host"))
    if bd == 8:
        sl = mr.sqrt_lambda(oracle, pc.QP, 8)
        pc.check_constructed(res["default"][0], res["default"][1], res["amp1"][0], res["amp0"][0], lambda vx, vy: mr.qpel_cost(4 * vx, 4 * vy, sl))


# ---- 6. the one-call host form --------------------------------------------------------------------------------------------------------------------------------

def test_p_shape_frame_equals_the_pipeline(torch_cuda):
    res = pipeline(torch_cuda, 8)
    flat, org, stride = res["planes"]
    c = capi.Context(pc.W, pc.H, 8)
    before = c.stats()
    for name, rule in zip(("default", "amp0"), (None, pc.rules()[2])):
        got = c.p_shape_frame(flat[1], flat[0], org, stride, qp=pc.QP, search_range=pc.RANGE, rule=rule)
        sr.same(got, res[name][0], name)
    after = c.stats()
    assert after["bytes_d2h"] - before["bytes_d2h"] == 2 * c.num_ctus * 85 * 16
    assert after["bytes_h2d"] - before["bytes_h2d"] == 2 * 2 * pc.W * pc.H * 2
    for bad in (dict(qp=52), dict(search_range=0), dict(search_range=65), dict(rule=capi.pu_shape_rule(0, 0, 2))):
        with pytest.raises(capi.FastHevcError):
            c.p_shape_frame(flat[1], flat[0], org, stride, **dict(dict(qp=pc.QP, search_range=pc.RANGE), **bad))
    c.close()


# ---- 7. rejected calls ------------------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(torch_cuda, ctx):
    torch = torch_cuda
    ins, rules, _, _ = random_case()
    held = [to_dev(torch, a) for a in ins]
    shapes, costs = Guarded(torch, 2 * N * 85 * 16), Guarded(torch, 2 * N * 85 * 32)
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, nodes=held[0].data_ptr(), pus=held[1].data_ptr(), small=held[2].data_ptr(), P=2, rb=0, re=CH, rule=rules["amp1"], shapes=shapes.ptr)
    mk = capi.pu_shape_rule
    bad = [(dict(ctx=None), None), (dict(nodes=None), "argument"), (dict(pus=None), "argument"), (dict(shapes=None), "argument"),
           (dict(P=0), "layout"), (dict(P=-3), "layout"), (dict(rb=-1), "band"), (dict(re=CH + 1), "band"), (dict(rb=2, re=1), "band"),
           (dict(rule=mk([0, 0, 0, -1], 0, 1)), "margin_q8"), (dict(rule=mk([65536, 0, 0, 0], 0, 1)), "margin_q8"), (dict(rule=mk(0, [0, -1, 0, 0], 1)), "margin_abs"),
           (dict(rule=mk(0, 0, 2)), "amp_mode"), (dict(rule=mk(0, 0, -1)), "amp_mode"),
           (dict(P=(1 << 31) // N + 1), "CTUs")]
    launched = ctx.stats()["kernels_launched"]
    for change, text in bad:
        a = dict(good, **change)
        rc = lib.fhevc_pu_shape_select_device(a["ctx"], a["nodes"], a["pus"], a["small"], a["P"], a["rb"], a["re"], C.byref(a["rule"]), a["shapes"], costs.ptr, None)
        assert rc == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert shapes.untouched() and costs.untouched() and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted (rule, d_pus_small and d_costs NULL)
    assert lib.fhevc_pu_shape_select_device(ctx.h, good["nodes"], good["pus"], None, 2, 0, CH, None, shapes.ptr, None, None) == capi.OK
    torch.cuda.synchronize()
    assert costs.untouched() and not shapes.untouched()


# ---- 8. the timing slot -----------------------------------------------------------------------------------------------------------------------------------------

def test_slot_13_counts_one_launch_per_call(torch_cuda, ctx):
    torch = torch_cuda
    ins, rules, _, _ = random_case()
    held = [to_dev(torch, a) for a in ins]
    shapes = Guarded(torch, 2 * N * 85 * 16)
    torch.cuda.synchronize()
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(13, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls in (1, 2, 3):
        ctx.pu_shape_select_device(held[0].data_ptr(), held[1].data_ptr(), held[2].data_ptr(), 2, shapes.ptr, rule=rules["amp0"])
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(13)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (5, 11, 12))
    ctx.enable_kernel_timing(False)
    with pytest.raises(capi.FastHevcError):
        ctx.kernel_timing(14)
