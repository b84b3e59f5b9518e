"""The tree decision on the device: fhevc_p_tree_select_device (k_p_tree.hip) and fhevc_p_tree_frame, bit for bit -- every byte of both maps and every
field of every record, nothing sampled.  Expected values come from the Python restatement tests/p_tree_ref.py (pinned to hand-computed cases by
tests/test_p_tree_ref.py) and are cross-checked against the library's host function; nothing is compared with the kernel's own output except where two
launches must give the same bytes (unaligned pointers, repeated pictures).

The decision needs no planes: its contexts are 200 x 136 = 4 x 3 CTUs, ragged on both sides by 8 samples, and 100 x 76 = 2 x 2 CTUs, ragged by 36 and 12
(valid sizes that are no multiple of 8).  The chains run on the 104 x 88 pair of tests/p_tree_cases.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import p_tree_cases as tc
import p_tree_ref as tr
from fasthevc_amd import capi
from motion_gpu_helpers import CANARY, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

CONTEXTS = {"200x136": (200, 136, 2), "100x76": (100, 76, 6)}       # width, height, pictures of the random case
SDT, TDT, MDT = capi.SHAPE_DTYPE, capi.TREE_DTYPE, capi.MOTION_DTYPE
PER = (85, 124, 384)
ALL = (True, True, True)
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


def random_case(name):
    """random records of a context, four rules, and their expected records and maps; computed once"""
    if name not in _CACHE:
        W, H, P = CONTEXTS[name]
        n = ((W + 63) // 64) * ((H + 63) // 64)
        rng = np.random.default_rng(811)
        shapes = tr.random_shapes(rng, P, n)
        rules = {"default": capi.p_tree_rule_default(), "r1": tr.random_rule(rng), "r2": tr.random_rule(rng), "r3": tr.random_rule(rng)}
        exp = {k: tr.select(shapes, W, H, rule=r) for k, r in rules.items()}
        _CACHE[name] = (shapes, rules, exp)
    return _CACHE[name]


def band(a, rows, cw):
    return np.ascontiguousarray(a[:, rows[0] * cw:rows[1] * cw])


def run(torch, ctx, shapes, rule, rows=None, want=ALL, in_offset=0, map_offset=0, tree_offset=0, stream=None):
    """one call, then a synchronise -> (records [P, band CTUs, 85], depth_min, depth_max [P, band CTUs, 256]), None for an output not asked for; guards
    checked, and an output that was not asked for stays untouched"""
    P, nb = shapes.shape[:2]
    held = at_offset(torch, shapes, in_offset)
    dmin, dmax, tree = Guarded(torch, P * nb * 256, map_offset), Guarded(torch, P * nb * 256, map_offset), Guarded(torch, P * nb * 85 * 16, tree_offset)
    torch.cuda.synchronize()
    ctx.p_tree_select_device(held[1], P, dmin.ptr if want[0] else None, dmax.ptr if want[1] else None, tree.ptr if want[2] else None, rows=rows, stream=stream,
                             rule=rule)
    torch.cuda.synchronize()
    for g, w in zip((dmin, dmax, tree), want):
        assert w or g.untouched()
    return (tree.result(TDT, (P, nb, 85)) if want[2] else None, dmin.result(np.uint8, (P, nb, 256)) if want[0] else None,
            dmax.result(np.uint8, (P, nb, 256)) if want[1] else None)


def same_all(got, exp, what):
    if got[0] is not None:
        tr.same(got[0], exp[0], what)
    for i, n in ((1, "depth_min"), (2, "depth_max")):
        if got[i] is not None:
            assert np.array_equal(got[i], exp[i]), (what, n, np.argwhere(got[i] != exp[i])[:5])


@pytest.fixture(scope="module")
def contexts(torch_cuda):
    cs = {name: capi.Context(W, H, 8) for name, (W, H, _) in CONTEXTS.items()}
    yield cs
    for c in cs.values():
        c.close()


# ---- (a) random records: the restatement, the host function, the kernel ------------------------------------------------------------------------------

def test_the_random_draw_reaches_every_case():
    seen = None
    for name in CONTEXTS:
        _, _, exp = random_case(name)
        for rec, dmin, dmax in exp.values():
            seen = tr.coverage(rec, seen)
            assert (dmin <= dmax).all()
    assert tr.covers_everything(seen), seen


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_random_records_equal_the_restatement_and_the_host_function(torch_cuda, contexts, name):
    W, H, P = CONTEXTS[name]
    shapes, rules, exp = random_case(name)
    ctx = contexts[name]
    for rname, rule in rules.items():
        for p in range(P):
            hmin, hmax, hrec = capi.p_tree_select(shapes[p], W, H, rule, with_tree=True)
            same_all((hrec, hmin, hmax), tuple(e[p] for e in exp[rname]), ("host", rname, p))
        same_all(run(torch_cuda, ctx, shapes, rule), exp[rname], ("device", name, rname))
    # every combination of NULL outputs
    for want in itertools.product((True, False), repeat=3):
        if any(want) and want != ALL:
            same_all(run(torch_cuda, ctx, shapes, rules["r2"], want=want), exp["r2"], ("device", name, want))
    # rule NULL is the documented default
    same_all(run(torch_cuda, ctx, shapes, None), exp["default"], "rule NULL")


# ---- (b) unaligned pointers give the same bytes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_pointers_give_the_same_bytes(torch_cuda, contexts, offset):
    """d_shapes and d_tree 4, 8, 12 bytes behind a 16-byte boundary (dword loads; dword stores of the records), the maps 1, 2, 3 bytes (byte stores)"""
    shapes, rules, exp = random_case("200x136")
    ctx = contexts["200x136"]
    aligned = run(torch_cuda, ctx, shapes, rules["r1"])
    same_all(aligned, exp["r1"], "aligned")
    for kw in (dict(in_offset=4 * offset), dict(tree_offset=4 * offset), dict(map_offset=offset),
               dict(in_offset=4 * offset, tree_offset=16 - 4 * offset, map_offset=offset)):
        got = run(torch_cuda, ctx, shapes, rules["r1"], **kw)
        assert all(g.tobytes() == a.tobytes() for g, a in zip(got, aligned)), kw


# ---- (c) bands and extents ---------------------------------------------------------------------------------------------------------------------------------

def test_bands_and_extents(torch_cuda, contexts):
    torch = torch_cuda
    W, H, P = CONTEXTS["200x136"]
    shapes, rules, exp = random_case("200x136")
    ctx = contexts["200x136"]
    for rows in ((0, 3), (1, 2), (1, 3)):          # the guards are checked inside run()
        b = band(shapes, rows, 4)
        got = run(torch, ctx, b, rules["r3"], rows=rows)
        # a band's CTUs keep their place in the picture: the expected values of the band are the band of the expected values
        x = tr.select(b, W, H, rows=rows, rule=rules["r3"])
        same_all(x, tuple(band(e, rows, 4) for e in exp["r3"]), rows)
        same_all(got, x, rows)
    # an empty band writes nothing and launches nothing
    held = to_dev(torch, shapes)
    outs = [Guarded(torch, 4096) for _ in range(3)]
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.p_tree_select_device(held.data_ptr(), P, outs[0].ptr, outs[1].ptr, outs[2].ptr, rows=(2, 2))
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs) and ctx.stats()["kernels_launched"] == launched


def test_more_ctus_than_the_persistent_grid(torch_cuda, contexts):
    """700 pictures that repeat the two random ones = 8 400 CTUs in one launch, more than the grid's cap of eight workgroups of four waves on each of 256
    CUs: every repeat equals the first two pictures, and those equal the restatement"""
    shapes, rules, exp = random_case("200x136")
    P = 700
    assert P * 12 > 8 * 4 * 256
    got = run(torch_cuda, contexts["200x136"], np.tile(shapes, (P // 2, 1, 1)), rules["r2"])
    same_all(tuple(g[:2] for g in got), exp["r2"], "first pictures")
    for g in got:
        first = g[:2].tobytes()
        for p in range(2, P, 2):
            assert g[p:p + 2].tobytes() == first, p


# ---- (d) the rule is per call: two streams -----------------------------------------------------------------------------------------------------------------

def test_two_rules_in_flight_on_two_streams(torch_cuda, contexts):
    torch = torch_cuda
    shapes, rules, exp = random_case("200x136")
    ctx = contexts["200x136"]
    assert not np.array_equal(exp["r1"][2], exp["r3"][2]) or not np.array_equal(exp["r1"][1], exp["r3"][1])
    held = to_dev(torch, shapes)
    n = shapes.shape[0] * shapes.shape[1]
    outs = [(Guarded(torch, n * 256), Guarded(torch, n * 256), Guarded(torch, n * 85 * 16)) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    scratch = capi.PTreeRule()
    for name, s, o in (("r1", streams[0], outs[0]), ("r3", streams[1], outs[1])):
        C.memmove(C.byref(scratch), C.byref(rules[name]), C.sizeof(scratch))
        ctx.p_tree_select_device(held.data_ptr(), shapes.shape[0], o[0].ptr, o[1].ptr, o[2].ptr, stream=s.cuda_stream, rule=scratch)
        C.memset(C.byref(scratch), 0, C.sizeof(scratch))      # the rule was read during the call
    torch.cuda.synchronize()
    for name, o in zip(("r1", "r3"), outs):
        shp = shapes.shape[:2]
        same_all((o[2].result(TDT, shp + (85,)), o[0].result(np.uint8, shp + (256,)), o[1].result(np.uint8, shp + (256,))), exp[name], name)


# ---- (e) the real chains on one stream, no host synchronisation ------------------------------------------------------------------------------------------------

def chains(torch):
    """the constructed pair as uint8 planes; per chain ("wide": zero-centred, "centred": coarse range 4) everything queued on ONE stream with no host
    synchronisation in between -> {chain: dict(centres, shapes, tree, dmin, dmax)}; computed once"""
    if "chains" not in _CACHE:
        cur, ref = tc.pictures()
        W, H, qp, R = tc.W, tc.H, tc.QP, tc.RANGE
        d_luma = to_dev(torch, np.stack([ref, cur]))
        c = capi.Context(W, H, 8, max_frames=2)
        n = c.num_ctus
        res = {}
        for chain in ("wide", "centred"):
            cen = Guarded(torch, n * 16)
            found = [Guarded(torch, n * k * 16) for k in PER]
            fine = [Guarded(torch, n * k * 16) for k in PER]
            shapes, tree, dmin, dmax = Guarded(torch, n * 85 * 16), Guarded(torch, n * 85 * 16), Guarded(torch, n * 256), Guarded(torch, n * 256)
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            s, p = st.cuda_stream, d_luma.data_ptr()
            if chain == "centred":
                c.motion_centres_device(p, 1, W, W * H, 2, cen.ptr, stream=s, qp=qp, coarse_range=tc.COARSE)
                c.motion_search_pu_centred_device(p, 1, W, W * H, 2, cen.ptr, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
                c.motion_refine_pu_centred_device(p, 1, W, W * H, 2, cen.ptr, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr,
                                                  stream=s, qp=qp, max_range=R)
            else:
                c.motion_search_pu_wide_device(p, 1, W, W * H, 2, found[0].ptr, found[1].ptr, found[2].ptr, stream=s, qp=qp, search_range=R)
                c.motion_refine_pu_wide_device(p, 1, W, W * H, 2, found[0].ptr, fine[0].ptr, found[1].ptr, fine[1].ptr, found[2].ptr, fine[2].ptr, stream=s, qp=qp,
                                               max_range=R)
            c.pu_shape_select_device(fine[0].ptr, fine[1].ptr, fine[2].ptr, 1, shapes.ptr, stream=s)
            c.p_tree_select_device(shapes.ptr, 1, dmin.ptr, dmax.ptr, tree.ptr, stream=s)
            torch.cuda.synchronize()
            res[chain] = dict(centres=cen.result(MDT, (n,)) if chain == "centred" else None, shapes=shapes.result(SDT, (n, 85)), tree=tree.result(TDT, (n, 85)),
                              dmin=dmin.result(np.uint8, (n, 256)), dmax=dmax.result(np.uint8, (n, 256)))
            if chain == "wide":
                assert cen.untouched()
        c.close()
        _CACHE["chains"] = res
    return _CACHE["chains"]


@pytest.mark.parametrize("chain", ["centred", "wide"])
def test_chain_and_tree_on_one_stream(oracle, torch_cuda, chain):
    got = chains(torch_cuda)[chain]
    case = tc.centred_case(oracle) if chain == "centred" else tc.constructed_case(oracle)
    if chain == "centred":
        # the centre of CTU 0 first: everything behind it is priced relative to it
        for f in ("mvx", "mvy", "cost_best"):
            assert np.array_equal(got["centres"][f], case["centres"][f]), (f, got["centres"], case["centres"])
    for f in SDT.names:
        assert np.array_equal(got["shapes"][f], case["shapes"][f]), ("shapes", f)
    tr.same(got["tree"], case["tree"], chain)
    assert np.array_equal(got["dmin"], case["dmin"]) and np.array_equal(got["dmax"], case["dmax"])
    tc.check_constructed(got["tree"], got["dmin"], got["dmax"], case["vector_cost"])
    # ... and the library's host function on the device's records
    hmin, hmax, hrec = capi.p_tree_select(got["shapes"], tc.W, tc.H, with_tree=True)
    same_all((hrec, hmin, hmax), (got["tree"], got["dmin"], got["dmax"]), "host")


def test_the_pair_scaled_to_10_bit_through_the_host_form(torch_cuda):
    """the samples times four: every constructed block still refines to SATD 0 at its vector, so the map is the same"""
    cur, ref = tc.pictures()
    bc, org, stride = pel(cur.astype(np.int64) << 2)
    br, _, _ = pel(ref.astype(np.int64) << 2)
    c = capi.Context(tc.W, tc.H, 10)
    for coarse in (0, tc.COARSE):
        dmin, dmax, shapes = c.p_tree_frame(bc, br, org, stride, qp=tc.QP, search_range=tc.RANGE, coarse_range=coarse, with_shapes=True)
        erec, emin, emax = tr.select(shapes[None], tc.W, tc.H)
        assert np.array_equal(dmin, emin[0]) and np.array_equal(dmax, emax[0]) and np.array_equal(dmin, dmax)
        assert np.array_equal(dmin[0], tc.expected_map_ctu0()), (coarse, dmin[0].reshape(16, 16))
        assert erec["cost_tree"][0, 0, 0] < erec["cost_own"][0, 0, 0]
    c.close()


# ---- (f) the one-call host form --------------------------------------------------------------------------------------------------------------------------------

def test_p_tree_frame_equals_the_chains(torch_cuda):
    res = chains(torch_cuda)
    cur, ref = tc.pictures()
    bc, org, stride = pel(cur)
    br, _, _ = pel(ref)
    c = capi.Context(tc.W, tc.H, 8)
    n = c.num_ctus
    for coarse, chain in ((0, "wide"), (tc.COARSE, "centred")):
        before = c.stats()
        dmin, dmax, shapes = c.p_tree_frame(bc, br, org, stride, qp=tc.QP, search_range=tc.RANGE, coarse_range=coarse, with_shapes=True)
        assert dmin.tobytes() == res[chain]["dmin"].tobytes() and dmax.tobytes() == res[chain]["dmax"].tobytes()
        assert shapes.tobytes() == res[chain]["shapes"].tobytes()
        mid = c.stats()
        assert mid["bytes_d2h"] - before["bytes_d2h"] == n * (512 + 85 * 16)
        lo, hi = c.p_tree_frame(bc, br, org, stride, qp=tc.QP, search_range=tc.RANGE, coarse_range=coarse)          # shapes NULL: only the maps come back
        assert lo.tobytes() == dmin.tobytes() and hi.tobytes() == dmax.tobytes()
        assert c.stats()["bytes_d2h"] - mid["bytes_d2h"] == n * 512
    # the tree rule reaches the kernel: a wide split margin at level 0 forces no split of the whole CTU, and forbids none
    lo, hi = c.p_tree_frame(bc, br, org, stride, qp=tc.QP, search_range=tc.RANGE, tree_rule=capi.p_tree_rule(split_abs=[0x7FFFFFFF, 0, 0]))
    assert (lo[0] == 0).all() and hi.tobytes() == res["wide"]["dmax"].tobytes()
    c.close()


# ---- (g) rejected calls ------------------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(torch_cuda, contexts):
    torch = torch_cuda
    shapes, rules, _ = random_case("200x136")
    ctx = contexts["200x136"]
    P, n = shapes.shape[:2]
    held = to_dev(torch, shapes)
    outs = [Guarded(torch, P * n * 256), Guarded(torch, P * n * 256), Guarded(torch, P * n * 85 * 16)]
    torch.cuda.synchronize()
    lib = ctx.lib
    good = dict(ctx=ctx.h, shapes=held.data_ptr(), P=P, rb=0, re=3, rule=rules["r1"], o0=outs[0].ptr, o1=outs[1].ptr, o2=outs[2].ptr)
    mk = capi.p_tree_rule
    bad = [(dict(ctx=None), None), (dict(shapes=None), "argument"), (dict(o0=None, o1=None, o2=None), "argument"),
           (dict(P=0), "layout"), (dict(P=-3), "layout"), (dict(rb=-1), "band"), (dict(re=4), "band"), (dict(rb=2, re=1), "band"),
           (dict(rule=mk(split_q8=[0, 0, -1])), "split_q8"), (dict(rule=mk(split_q8=[65536, 0, 0])), "split_q8"), (dict(rule=mk(stop_q8=[0, -1, 0])), "stop_q8"),
           (dict(rule=mk(stop_q8=[0, 0, 65536])), "stop_q8"), (dict(rule=mk(split_abs=[0, -1, 0])), "split_abs"), (dict(rule=mk(stop_abs=[-1, 0, 0])), "stop_abs"),
           (dict(rule=mk(split_cost=[0, 0, -1])), "split_cost"), (dict(P=(1 << 31) // n + 1), "CTUs")]
    launched = ctx.stats()["kernels_launched"]
    for change, text in bad:
        a = dict(good, **change)
        rc = lib.fhevc_p_tree_select_device(a["ctx"], a["shapes"], a["P"], a["rb"], a["re"], C.byref(a["rule"]), a["o0"], a["o1"], a["o2"], None)
        assert rc == capi.E_INVALID, change
        if text:
            assert text in lib.fhevc_last_error(ctx.h).decode(), (change, lib.fhevc_last_error(ctx.h))
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs) and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted (rule NULL, one output)
    assert lib.fhevc_p_tree_select_device(ctx.h, good["shapes"], P, 0, 3, None, None, outs[1].ptr, None, None) == capi.OK
    torch.cuda.synchronize()
    assert outs[0].untouched() and outs[2].untouched() and not outs[1].untouched()
    # the frame form
    cur, ref = tc.pictures()
    bc, org, stride = pel(cur)
    br, _, _ = pel(ref)
    c = capi.Context(tc.W, tc.H, 8)
    launched = c.stats()["kernels_launched"]
    base = dict(qp=tc.QP, search_range=8, coarse_range=0)
    for change in (dict(search_range=9, coarse_range=1), dict(coarse_range=15), dict(coarse_range=-1), dict(search_range=0), dict(search_range=65), dict(qp=52),
                   dict(tree_rule=mk(stop_q8=[65536, 0, 0])), dict(shape_rule=capi.pu_shape_rule(0, 0, 2))):
        with pytest.raises(capi.FastHevcError):
            c.p_tree_frame(bc, br, org, stride, **dict(base, **change))
    canary = np.full(c.num_ctus * 256, CANARY, np.uint8)
    lo, hi = canary.copy(), canary.copy()
    rc = c.lib.fhevc_p_tree_frame(c.h, bc.ctypes.data + 2 * org, br.ctypes.data + 2 * org, stride, tc.QP, 9, 4, None, None, lo.ctypes.data, hi.ctypes.data, None)
    assert rc == capi.E_INVALID and (lo == CANARY).all() and (hi == CANARY).all() and c.stats()["kernels_launched"] == launched
    assert c.lib.fhevc_p_tree_frame(c.h, bc.ctypes.data + 2 * org, br.ctypes.data + 2 * org, stride, tc.QP, 8, 0, None, None, None, hi.ctypes.data, None) == capi.E_INVALID
    c.close()


# ---- (h) the timing slot -------------------------------------------------------------------------------------------------------------------------------------------

def test_slot_17_counts_one_launch_per_call(torch_cuda, contexts):
    torch = torch_cuda
    shapes, rules, _ = random_case("200x136")
    ctx = contexts["200x136"]
    held = to_dev(torch, shapes)
    out = Guarded(torch, shapes.shape[0] * shapes.shape[1] * 256)
    torch.cuda.synchronize()
    ctx.enable_kernel_timing(True)
    for s in (13, 15, 17):
        ctx.kernel_timing(s, reset=True)
    launched = ctx.stats()["kernels_launched"]
    for calls in (1, 2, 3):
        ctx.p_tree_select_device(held.data_ptr(), shapes.shape[0], out.ptr, rule=rules["r1"])
        torch.cuda.synchronize()
        ms, count = ctx.kernel_timing(17)
        assert count == calls and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + calls
    assert all(ctx.kernel_timing(s)[1] == 0 for s in (5, 13, 15))
    ctx.enable_kernel_timing(False)
    for s in (14, 16, 18):
        with pytest.raises(capi.FastHevcError):
            ctx.kernel_timing(s)
