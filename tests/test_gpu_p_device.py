"""Config 4 on the device: fhevc_p_depth_range_device (k_p_rule.hip) and fhevc_p_predict_frame, bit for bit (np.array_equal, no tolerance).

Every expected value comes from the CPU oracle (fho_p_depth_range, fho_p_node_depth, fho_p_motion_compensated_depth: the independent
restatement) and is cross-checked against the library's own host functions before anything is compared with the GPU; nothing is compared with
the kernel's own output.  So that a comparison cannot pass vacuously the synthetic test asserts on the ORACLE's result first: all four depths
occur in depth_max, depth_min < depth_max and depth_min == depth_max both occur (default rule, plausible nodes), depth_min reaches 3 under
t_split = 0 / window = 4, and the displaced modes differ from the co-located one.

Why the synthetic cases are a covering set and not a full cross product: 4 geometries x 2 picture counts x 3 modes x 4 QPs x 7 rules x 2 node
sets x 2 map kinds would be 2 688 oracle passes over up to 1 530 CTUs.  Every (geometry, mode, node set) runs all seven rules; QP, the number
of pictures and the kind of reference map rotate with the rule so that every value of each meets every geometry, mode and node set."""
import ctypes as C

import numpy as np
import pytest

from fasthevc_amd import capi, frames, weights
from oracle import oracle_py as op

pytestmark = pytest.mark.gpu

CANARY = 0xA5
MODES = ["colocated", "unit", "node"]
QPS = [0, 22, 37, 51]


# ---- generators (no GPU) ---------------------------------------------------------------------------------------------------------------------

def random_partition(rng, n):
    """a valid HM depth map per CTU (top-down random splits), as tests/test_host_logic.py builds them"""
    m = np.zeros((n, 16, 16), np.uint8)
    for c in range(n):
        if rng.random() < 0.3:
            continue
        for q in range(4):
            qy, qx = 8 * (q >> 1), 8 * (q & 1)
            if rng.random() < 0.4:
                m[c, qy:qy + 8, qx:qx + 8] = 1
                continue
            for b in range(4):
                by, bx = qy + 4 * (b >> 1), qx + 4 * (b & 1)
                m[c, by:by + 4, bx:bx + 4] = 2 if rng.random() < 0.5 else 3
    return m.reshape(n, 256)


def reference_maps(rng, kind, P, n):
    if kind == "bytes":
        return rng.integers(0, 4, size=(P, n, 256)).astype(np.uint8)
    return np.stack([random_partition(rng, n) for _ in range(P)])


NODE_LEVEL = np.array([0] + [1] * 4 + [2] * 16 + [3] * 64)
NODE_FIRST = [0, 1, 5, 21]


def node_geometry(W, H):
    """(x, y, size) [numCtus, 85] of every node, and which nodes cross the picture edge (the search flags those with 0xFFFFFFFF)"""
    cw, ch = frames.ctu_grid(W, H)
    x, y, s = np.zeros((cw * ch, 85), int), np.zeros((cw * ch, 85), int), np.zeros((cw * ch, 85), int)
    for c in range(cw * ch):
        for k in range(85):
            lvl = NODE_LEVEL[k]
            i = k - NODE_FIRST[lvl]
            s[c, k] = 64 >> lvl
            x[c, k] = (c % cw) * 64 + (i % (1 << lvl)) * s[c, k]
            y[c, k] = (c // cw) * 64 + (i // (1 << lvl)) * s[c, k]
    return x, y, s, (x + s > W) | (y + s > H)


def children(k):
    lvl = NODE_LEVEL[k]
    i = k - NODE_FIRST[lvl]
    nx, ny, per = i % (1 << lvl), i // (1 << lvl), 2 << lvl
    return [NODE_FIRST[lvl + 1] + (2 * ny + (j >> 1)) * per + 2 * nx + (j & 1) for j in range(4)]


def plausible_nodes(rng, P, W, H):
    """node set (a): distortion per sample from a gamma draw times the node's area, a parent a little above the sum of its children, cost_best
    slightly above satd_best, vectors within +-8 that children mostly inherit; nodes crossing the picture edge flagged as the search flags them"""
    *_, crossing = node_geometry(W, H)
    n = crossing.shape[0]
    out = np.zeros((P, n, 85), capi.MOTION_DTYPE)
    # the texture of a CTU varies from flat to busy: per-CTU scale over two decades, per-8x8 gamma around it
    scale = np.exp(rng.uniform(np.log(0.05), np.log(20.0), size=(P, n, 1)))
    best = np.zeros((P, n, 85))
    best[:, :, 21:] = rng.gamma(2.0, 0.5, size=(P, n, 64)) * scale * 64
    for k in range(20, -1, -1):
        best[:, :, k] = best[:, :, children(k)].sum(axis=2) * (1.0 + rng.uniform(0.0, 0.6, size=(P, n)) ** 2)
    out["satd_best"] = np.minimum(best, 2 ** 30).astype(np.uint32)
    out["satd_zero"] = np.minimum(best * (1.0 + rng.exponential(0.5, size=best.shape)), 2 ** 30).astype(np.uint32)
    out["cost_best"] = out["satd_best"] + rng.integers(0, 40, size=best.shape).astype(np.uint32)
    mv = rng.integers(-8, 9, size=(P, n, 85, 2))
    for k in range(21):
        for ck in children(k):
            keep = rng.random((P, n)) < 0.6
            mv[:, :, ck][keep] = mv[:, :, k][keep]
    out["mvx"], out["mvy"] = mv[..., 0], mv[..., 1]
    for f in ("satd_zero", "satd_best", "cost_best"):
        out[f][:, crossing] = 0xFFFFFFFF
    out["mvx"][:, crossing] = 0
    out["mvy"][:, crossing] = 0
    return out


def wild_nodes(rng, P, W, H):
    """node set (b): uniformly random 32-bit fields, 20 % of cost_best at 0xFFFFFFFF, vectors over the full int16 range: the wrapping sums of the
    rule and the position clamps of the displaced modes"""
    n = frames.ctu_grid(W, H)[0] * frames.ctu_grid(W, H)[1]
    out = np.zeros((P, n, 85), capi.MOTION_DTYPE)
    for f in ("satd_zero", "satd_best", "cost_best"):
        out[f] = rng.integers(0, 1 << 32, size=(P, n, 85), dtype=np.uint64).astype(np.uint32)
    out["cost_best"][rng.random((P, n, 85)) < 0.2] = 0xFFFFFFFF
    out["mvx"] = rng.integers(-32768, 32768, size=(P, n, 85)).astype(np.int16)
    out["mvy"] = rng.integers(-32768, 32768, size=(P, n, 85)).astype(np.int16)
    out["mvx"][rng.random((P, n, 85)) < 0.02] = -32768
    out["mvy"][rng.random((P, n, 85)) < 0.02] = 32767
    return out


def rules():
    """(name, PRule): default, wide, both with t_split = 0 and window = 4, windows 0 and 2, seeded random weights of the shipped magnitude"""
    def variant(base, **kw):
        r = base()
        for k, v in kw.items():
            if k == "window":
                r.window = v
            else:
                for i in range(3):
                    getattr(r, k)[i] = v
        return r
    rnd = capi.p_rule_default()
    rng = np.random.default_rng(77)
    for lvl in range(3):
        for i in range(9):
            rnd.w[lvl][i] = int(rng.integers(-6000, 6001))
        rnd.w[lvl][9] = int(rng.integers(-450000, 450001))
        rnd.t_split[lvl] = int(rng.integers(0, 1 << 20))
        rnd.t_stop[lvl] = int(rng.integers(0, 1 << 20))
    rnd.window = 3
    return [("default", capi.p_rule_default()), ("wide", capi.p_rule_default_wide()),
            ("default-open", variant(capi.p_rule_default, t_split=0, window=4)), ("wide-open", variant(capi.p_rule_default_wide, t_split=0, window=4)),
            ("window0", variant(capi.p_rule_default, window=0)), ("window2", variant(capi.p_rule_default, window=2)), ("random", rnd)]


# ---- the expected maps: oracle, cross-checked against the library's host functions ------------------------------------------------------------

def expected(oracle, nodes, maps, W, H, rows, qp, mode, rule):
    """nodes [P, band CTUs, 85], maps [P, numCtus, 256] -> (depth_min, depth_max) [P, band CTUs, 256] from the oracle; the library's host
    functions must give the same (asserted here)"""
    lib = capi.load_library()
    cw, ch = frames.ctu_grid(W, H)
    rb, re = rows
    P, nb = nodes.shape[0], (re - rb) * cw
    assert nodes.shape == (P, nb, 85) and maps.shape == (P, cw * ch, 256)
    for f in (oracle.fho_p_motion_compensated_depth, oracle.fho_p_node_depth):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        f.restype = None
    orule = op.PRule()   # the oracle's own mirror of the struct, filled with the same bytes
    C.memmove(C.byref(orule), C.byref(rule), C.sizeof(rule))
    dmin, dmax = np.zeros((P, nb, 256), np.uint8), np.zeros((P, nb, 256), np.uint8)
    hmin, hmax = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    seen, hseen = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    for p in range(P):
        pm = np.ascontiguousarray(maps[p])
        for i in range(nb):
            ctu = rb * cw + i
            nd = np.ascontiguousarray(nodes[p, i])
            vw, vh = min(64, W - (ctu % cw) * 64), min(64, H - (ctu // cw) * 64)
            if mode == "colocated":
                seen[:] = pm[ctu]
                hseen[:] = pm[ctu]
            elif mode == "unit":
                oracle.fho_p_motion_compensated_depth(nd.ctypes.data, pm.ctypes.data, W, H, ctu, seen.ctypes.data)
                assert lib.fhevc_p_motion_compensated_depth(nd.ctypes.data, pm.ctypes.data, W, H, ctu, hseen.ctypes.data) == capi.OK
            else:
                oracle.fho_p_node_depth(nd.ctypes.data, pm.ctypes.data, W, H, ctu, seen.ctypes.data)
                assert lib.fhevc_p_node_depth(nd.ctypes.data, pm.ctypes.data, W, H, ctu, hseen.ctypes.data) == capi.OK
            oracle.fho_p_depth_range(nd.ctypes.data, seen.ctypes.data, vw, vh, qp, C.byref(orule), dmin[p, i].ctypes.data, dmax[p, i].ctypes.data)
            assert lib.fhevc_p_depth_range(nd.ctypes.data, hseen.ctypes.data, vw, vh, qp, C.byref(rule), hmin.ctypes.data, hmax.ctypes.data) == capi.OK
            assert np.array_equal(hseen, seen) and np.array_equal(hmin, dmin[p, i]) and np.array_equal(hmax, dmax[p, i]), \
                f"the host functions and the oracle disagree (picture {p}, CTU {ctu}, {mode})"
    return dmin, dmax


def band_of(a, W, H, rows):
    """[P, numCtus, ...] -> the CTUs of rows [rb, re)"""
    cw = frames.ctu_grid(W, H)[0]
    return np.ascontiguousarray(a[:, rows[0] * cw:rows[1] * cw])


def inside_mask(W, H, rows):
    """[band CTUs, 256] bool: units inside the picture"""
    cw, ch = frames.ctu_grid(W, H)
    m = np.zeros((ch * cw, 16, 16), bool)
    for c in range(cw * ch):
        m[c, :min(16, (H - (c // cw) * 64 + 3) // 4), :min(16, (W - (c % cw) * 64 + 3) // 4)] = True
    return m.reshape(cw * ch, 256)[rows[0] * cw:rows[1] * cw]


# ---- device plumbing -------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


class Guarded:
    """nbytes of device output between two canary-filled guards of 4 KiB, everything pre-filled with the canary"""
    GUARD = 4096

    def __init__(self, torch, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * self.GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + self.GUARD

    def result(self, shape):
        """the payload; asserts that both guards still hold the canary"""
        h = self.t.cpu().numpy()
        assert (h[:self.GUARD] == CANARY).all() and (h[self.GUARD + self.n:] == CANARY).all(), "a guard around the output was written"
        return h[self.GUARD:self.GUARD + self.n].reshape(shape)

    def untouched(self):
        return bool((self.t.cpu().numpy() == CANARY).all())


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def run_device(torch, ctx, nodes, maps, rows, qp, mode, rule, stream=None, want_max=True):
    """one call on `stream` (None: the NULL stream), then a synchronise -> (depth_min, depth_max or None), guards checked"""
    P, nb = nodes.shape[:2]
    d_nodes, d_maps = to_dev(torch, nodes), to_dev(torch, maps)
    omin, omax = Guarded(torch, P * nb * 256), Guarded(torch, P * nb * 256)
    torch.cuda.synchronize()
    ctx.p_depth_range_device(d_nodes.data_ptr(), d_maps.data_ptr(), P, omin.ptr, omax.ptr if want_max else None, rows=rows, qp=qp,
                             prev_mode=mode, rule=rule, stream=stream)
    torch.cuda.synchronize()
    return omin.result((P, nb, 256)), (omax.result((P, nb, 256)) if want_max else None)


# ---- 1. synthetic nodes, every mode and rule ----------------------------------------------------------------------------------------------------

GEOMETRIES = [(64, 64, None), (416, 240, None), (1920, 1080, None), (3840, 2160, (30, 34))]
GEOMETRY_IDS = ["64x64", "416x240", "1920x1080", "3840x2160-rows30-34"]


@pytest.mark.parametrize("node_set", ["plausible", "wild"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEOMETRY_IDS)
def test_synthetic_nodes_every_mode_and_rule(oracle, torch_cuda, geometry, mode, node_set):
    torch = torch_cuda
    W, H, rows = geometry
    cw, ch = frames.ctu_grid(W, H)
    rows = rows or (0, ch)
    case = GEOMETRIES.index(geometry) * 6 + MODES.index(mode) * 2 + (node_set == "wild")
    rng = np.random.default_rng(1000 + case)
    make = plausible_nodes if node_set == "plausible" else wild_nodes
    ctx = capi.Context(W, H, 8)
    # the oracle's side first, for every run of this case
    runs = []
    for i, (name, rule) in enumerate(rules()):
        P = 3 if (i + case) % 2 else 1
        qp = QPS[(i + case) % 4]
        kind = "partition" if mode == "node" or (i + case // 2) % 2 == 0 else "bytes"
        nodes = band_of(make(rng, P, W, H), W, H, rows)
        maps = reference_maps(rng, kind, P, cw * ch)
        emin, emax = expected(oracle, nodes, maps, W, H, rows, qp, mode, rule)
        runs.append((name, rule, P, qp, kind, nodes, maps, emin, emax))
        inside = inside_mask(W, H, rows)
        assert (emin <= emax).all() and emax.max() <= 3 and not emax[:, ~inside].any()
        if node_set == "plausible" and cw * ch >= 28:   # a single CTU cannot be asked to show every outcome
            if name == "default":
                assert set(np.unique(emax[:, inside])) == {0, 1, 2, 3}, "depth_max of the oracle does not show all four depths"
                assert (emin < emax).any() and (emin[:, inside] == emax[:, inside]).any()
            if name == "default-open":
                assert emin.max() == 3, "depth_min of the oracle never reaches 3 under t_split = 0, window = 4"
            if mode != "colocated" and name in ("default", "wide-open"):
                cmin, cmax = expected(oracle, nodes, maps, W, H, rows, qp, "colocated", rule)
                assert not (np.array_equal(cmin, emin) and np.array_equal(cmax, emax)), "the displaced mode equals the co-located one"
    # then the GPU
    for name, rule, P, qp, kind, nodes, maps, emin, emax in runs:
        gmin, gmax = run_device(torch, ctx, nodes, maps, rows, qp, mode, rule)
        what = (name, P, qp, kind)
        assert np.array_equal(gmin, emin), (what, "depth_min", np.argwhere(gmin != emin)[:5])
        assert np.array_equal(gmax, emax), (what, "depth_max", np.argwhere(gmax != emax)[:5])
    ctx.close()


# ---- 2. real nodes, no host in between ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("search", ["range4-satd-default-colocated", "range64-sad-wide-node"])
def test_real_nodes_no_host_in_between(oracle, torch_cuda, search):
    """The 1080p pan clip, 4 pictures: classifier (the reference maps), motion search and the P decision queued on ONE stream with no synchronise
    between them -- on the NULL stream and on a caller's non-blocking stream, from uint8 and from int16 planes -- equal the host route on the
    downloaded nodes and maps."""
    torch = torch_cuda
    W, H, NF, qp = 1920, 1080, 4, 32
    wide = search.startswith("range64")
    rng_, mode, rule = (64, "node", capi.p_rule_default_wide()) if wide else (4, "colocated", capi.p_rule_default())
    ys = frames.pan_clip(W, H, NF, v_structure=21, v_noise=-37) if wide else frames.pan_clip(W, H, NF)
    ctx = capi.Context(W, H, 8, weights.random_weights(3), max_frames=NF)
    if wide:
        ctx.set_motion_distortion("sad")
    n = ctx.num_ctus
    planes = [frames.to_pel_plane(y, 8) for y in ys]
    org, stride, fs = planes[0][1], planes[0][2], planes[0][0].size
    d8 = torch.from_numpy(np.stack(ys)).cuda()
    d16 = torch.from_numpy(np.stack([p[0] for p in planes])).cuda()
    layouts = {"uint8": (d8.data_ptr(), 1, W, W * H), "int16": (d16.data_ptr() + 2 * org, 2, stride, fs)}
    side = torch.cuda.Stream()
    results = {}
    for lname, (ptr, sb, st, fstride) in layouts.items():
        for sname, stream in (("null", None), ("own", side)):
            d_maps = torch.full((NF * n * 256,), CANARY, dtype=torch.uint8, device="cuda")
            d_nodes = torch.full(((NF - 1) * n * 85 * 16,), CANARY, dtype=torch.uint8, device="cuda")
            omin, omax = Guarded(torch, (NF - 1) * n * 256), Guarded(torch, (NF - 1) * n * 256)
            torch.cuda.synchronize()
            s = None if stream is None else stream.cuda_stream
            # pictures 0 .. NF-2 are the reference pictures of P pictures 1 .. NF-1: map p of the classifier's output is the map of picture p
            ctx.predict_frames_device(ptr, sb, st, fstride, NF, d_maps.data_ptr(), stream=s, qp=qp)
            ctx.motion_search_device(ptr, sb, st, fstride, NF, d_nodes.data_ptr(), stream=s, qp=qp, search_range=rng_)
            ctx.p_depth_range_device(d_nodes.data_ptr(), d_maps.data_ptr(), NF - 1, omin.ptr, omax.ptr, stream=s, qp=qp, prev_mode=mode, rule=rule)
            torch.cuda.synchronize()
            results[(lname, sname)] = (d_nodes.cpu().numpy().view(capi.MOTION_DTYPE).reshape(NF - 1, n, 85),
                                       d_maps.cpu().numpy().reshape(NF, n, 256), omin.result((NF - 1, n, 256)), omax.result((NF - 1, n, 256)))
    nodes, maps, _, _ = results[("int16", "null")]
    assert (maps <= 3).all() and len(np.unique(maps)) > 1 and (nodes["mvx"] != 0).any()
    emin, emax = expected(oracle, nodes, maps[:NF - 1], W, H, (0, ctx.ctus_y), qp, mode, rule)
    assert (emin < emax).any()
    for key, (gn, gm, gmin, gmax) in results.items():
        assert all(np.array_equal(gn[k], nodes[k]) for k in capi.MOTION_DTYPE.names) and np.array_equal(gm, maps), key
        assert np.array_equal(gmin, emin) and np.array_equal(gmax, emax), key
    ctx.close()


# ---- 3. bands and extents ------------------------------------------------------------------------------------------------------------------------

def test_bands_and_extents(oracle, torch_cuda):
    torch = torch_cuda
    W, H, P, qp = 1920, 1080, 2, 30
    cw, ch = frames.ctu_grid(W, H)
    rng = np.random.default_rng(31)
    nodes, maps = plausible_nodes(rng, P, W, H), reference_maps(rng, "partition", P, cw * ch)
    ctx = capi.Context(W, H, 8)
    for mode in MODES:
        rule = capi.p_rule_default()
        emin, emax = expected(oracle, nodes, maps, W, H, (0, ch), qp, mode, rule)
        fmin, fmax = run_device(torch, ctx, nodes, maps, (0, ch), qp, mode, rule)
        assert np.array_equal(fmin, emin) and np.array_equal(fmax, emax), mode
        for rows in ((14, 17), (0, 5)):
            bmin, bmax = run_device(torch, ctx, band_of(nodes, W, H, rows), maps, rows, qp, mode, rule)   # guards checked inside
            assert np.array_equal(bmin, band_of(emin, W, H, rows)) and np.array_equal(bmax, band_of(emax, W, H, rows)), (mode, rows)
        # depth_max is optional: depth_min is the same without it
        nmin, _ = run_device(torch, ctx, nodes, maps, (0, ch), qp, mode, rule, want_max=False)
        assert np.array_equal(nmin, emin), mode
    # an empty band writes nothing and succeeds
    d_nodes, d_maps = to_dev(torch, nodes), to_dev(torch, maps)
    omin, omax = Guarded(torch, 4096), Guarded(torch, 4096)
    torch.cuda.synchronize()
    launched = ctx.stats()["kernels_launched"]
    ctx.p_depth_range_device(d_nodes.data_ptr(), d_maps.data_ptr(), P, omin.ptr, omax.ptr, rows=(7, 7), qp=qp)
    torch.cuda.synchronize()
    assert omin.untouched() and omax.untouched() and ctx.stats()["kernels_launched"] == launched
    # the launch is counted, and timed under which = 5
    ctx.enable_kernel_timing(True)
    ctx.kernel_timing(5, reset=True)
    ctx.p_depth_range_device(d_nodes.data_ptr(), d_maps.data_ptr(), P, omin.ptr, None, rows=(0, 1), qp=qp)
    torch.cuda.synchronize()
    ms, count = ctx.kernel_timing(5)
    assert count == 1 and ms > 0.0 and ctx.stats()["kernels_launched"] == launched + 1
    ctx.enable_kernel_timing(False)
    ctx.close()


# ---- 4. the rule is per call -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("streams", ["one-stream", "two-streams"])
def test_the_rule_is_per_call(oracle, torch_cuda, streams):
    """Two calls with different rules back to back, no synchronise between them, separate outputs: each output matches its own rule.  The rule
    structs are overwritten on the host right after each call returns: the library must have read them during the call."""
    torch = torch_cuda
    W, H, P, qp = 1920, 1080, 3, 27
    cw, ch = frames.ctu_grid(W, H)
    rng = np.random.default_rng(41)
    nodes, maps = plausible_nodes(rng, P, W, H), reference_maps(rng, "partition", P, cw * ch)
    by_name = dict(rules())
    ra, rb = by_name["default"], by_name["wide-open"]
    ea, eb = expected(oracle, nodes, maps, W, H, (0, ch), qp, "unit", ra), expected(oracle, nodes, maps, W, H, (0, ch), qp, "unit", rb)
    assert not np.array_equal(ea[0], eb[0]) and not np.array_equal(ea[1], eb[1])
    ctx = capi.Context(W, H, 8)
    d_nodes, d_maps = to_dev(torch, nodes), to_dev(torch, maps)
    outs = [Guarded(torch, P * cw * ch * 256) for _ in range(4)]
    sa = torch.cuda.Stream()
    sb = torch.cuda.Stream() if streams == "two-streams" else sa
    torch.cuda.synchronize()
    scratch = capi.PRule()
    for rule, s, (omin, omax) in ((ra, sa, outs[:2]), (rb, sb, outs[2:])):
        C.memmove(C.byref(scratch), C.byref(rule), C.sizeof(rule))
        ctx.p_depth_range_device(d_nodes.data_ptr(), d_maps.data_ptr(), P, omin.ptr, omax.ptr, qp=qp, prev_mode="unit", rule=scratch, stream=s.cuda_stream)
        C.memset(C.byref(scratch), 0x7F, C.sizeof(scratch))
    torch.cuda.synchronize()
    shape = (P, cw * ch, 256)
    assert np.array_equal(outs[0].result(shape), ea[0]) and np.array_equal(outs[1].result(shape), ea[1])
    assert np.array_equal(outs[2].result(shape), eb[0]) and np.array_equal(outs[3].result(shape), eb[1])
    ctx.close()


# ---- 5. rejected calls -----------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(torch_cuda):
    torch = torch_cuda
    W, H = 416, 240
    ctx = capi.Context(W, H, 8)
    n = ctx.num_ctus
    d_nodes = torch.zeros((n * 85 * 16,), dtype=torch.uint8, device="cuda")
    d_maps = torch.zeros((n * 256,), dtype=torch.uint8, device="cuda")
    omin, omax = Guarded(torch, n * 256), Guarded(torch, n * 256)
    torch.cuda.synchronize()
    lib, rule = ctx.lib, capi.p_rule_default()
    good = dict(ctx=ctx.h, nodes=d_nodes.data_ptr(), maps=d_maps.data_ptr(), P=1, rb=0, re=ctx.ctus_y, qp=32, mode=0, dmin=omin.ptr)
    bad = [dict(ctx=None), dict(nodes=None), dict(maps=None), dict(dmin=None), dict(P=0), dict(P=-3), dict(qp=-1), dict(qp=52), dict(mode=3), dict(mode=-1),
           dict(rb=-1), dict(re=ctx.ctus_y + 1), dict(rb=3, re=2)]
    launched = ctx.stats()["kernels_launched"]
    for change in bad:
        a = dict(good, **change)
        rc = lib.fhevc_p_depth_range_device(a["ctx"], a["nodes"], a["maps"], a["P"], a["rb"], a["re"], a["qp"], a["mode"], C.byref(rule), a["dmin"], omax.ptr, None)
        assert rc == capi.E_INVALID, change
    torch.cuda.synchronize()
    assert omin.untouched() and omax.untouched() and ctx.stats()["kernels_launched"] == launched
    # the same call with nothing wrong is accepted (rule NULL = the shipped rule, depth_max NULL)
    assert lib.fhevc_p_depth_range_device(ctx.h, good["nodes"], good["maps"], 1, 0, ctx.ctus_y, 32, 0, None, omin.ptr, None, None) == capi.OK
    torch.cuda.synchronize()
    assert omax.untouched() and not omin.untouched()
    ctx.close()


# ---- 6. the host form ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd,search_range,sad", [(8, 4, False), (10, 3, False), (8, 64, True), (10, 24, True)])
def test_p_predict_frame_host_form(oracle, bd, search_range, sad):
    """fhevc_p_predict_frame on a ragged picture equals the library's own search followed by the oracle's rule, in all three modes"""
    W, H, qp = 416, 240, 33
    cw, ch = frames.ctu_grid(W, H)
    ys = frames.pan_clip(W, H, 2, seed=50 + bd, v_structure=9 if sad else 3, v_noise=-14 if sad else -2)
    (rbuf, org, stride), (cbuf, _, _) = [frames.to_pel_plane(y, bd) for y in ys]
    if bd > 8:
        cbuf = (cbuf + np.random.default_rng(bd).integers(0, 1 << (bd - 8), size=cbuf.shape, dtype=np.int16)).astype(np.int16)
    rng = np.random.default_rng(60 + bd)
    prev = random_partition(rng, cw * ch)
    ctx = capi.Context(W, H, bd)
    if sad:
        ctx.set_motion_distortion("sad")
    nodes = ctx.motion_search(cbuf, rbuf, org, stride, qp=qp, search_range=search_range)
    assert (nodes["mvx"] != 0).any()
    for mode in MODES:
        rule = capi.p_rule_default_wide() if sad else capi.p_rule_default()
        emin, emax = expected(oracle, nodes[None], prev[None], W, H, (0, ch), qp, mode, rule)
        gmin, gmax = ctx.p_predict_frame(cbuf, rbuf, prev, org, stride, qp=qp, search_range=search_range, prev_mode=mode, rule=rule)
        assert np.array_equal(gmin, emin[0]) and np.array_equal(gmax, emax[0]), mode
    dmin, dmax = ctx.p_predict_frame(cbuf, rbuf, prev, org, stride, qp=qp, search_range=search_range)   # rule None = the shipped rule, co-located
    emin, emax = expected(oracle, nodes[None], prev[None], W, H, (0, ch), qp, "colocated", capi.p_rule_default())
    assert np.array_equal(dmin, emin[0]) and np.array_equal(dmax, emax[0])
    with pytest.raises(capi.FastHevcError):
        ctx.p_predict_frame(cbuf, rbuf, prev, org, stride, qp=qp, search_range=search_range, prev_mode=7)
    ctx.close()
