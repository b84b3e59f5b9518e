"""The stream and asynchrony contract of the *_device entry points (include/fasthevc.h), bit for bit against the CPU oracle.

What the header promises and every other GPU test hides behind torch.cuda.synchronize():
  * stream == NULL is the context's own BLOCKING stream: ordered after everything issued earlier on the legacy default stream and
    before everything issued later on it -- a caller on the default stream needs no synchronisation (case a);
  * a caller on its own non-blocking stream passes that stream and the work is ordered on it (case b);
  * the calls do not block the host (case c);
  * fhevc_set_cnn_arith / fhevc_set_motion_distortion take effect at the next launch, never under a queued one (case d);
  * state the context shares between streams is guarded: the layer path's activation tensors (case e), the vector-cost table of the
    wide motion search (case f), the weight images that fhevc_set_weights overwrites in place (case g).

The tool is a bounded delay (torch.cuda._sleep, a spinning kernel) queued in front of the work under test: an ordering fault only shows
while the device is behind the host.  Behind the delay a producer copies the real planes over poison, the library runs, a consumer
copies the outputs away and the planes are poisoned again; ONE torch.cuda.synchronize() ends the test.  A library that ran early reads
poison, one that ran late delivers the canary, and both differ from the oracle.  Every buffer stays allocated for the whole test, so a
wrong ordering shows as wrong integers, never as a bad address; at most two caller streams exist per process.

Sizing of the delay, measured on an MI355X (torch 2.10 / ROCm 7.0; the counter behind torch.cuda._sleep ran at 2.4 GHz there: _sleep(64 000 000)
took 26.7 ms, and `delay_cycles` measures that rate again in every run instead of assuming it):
  * the host needs 0.25 - 0.33 ms for fhevc_set_weights of an FHW1 blob on an idle device (ten calls; the longest single call a test makes behind
    a delay), 0.004 - 0.008 ms to issue one fhevc_predict_frames_device, and 0.02 - 0.6 ms (time.perf_counter) to issue everything a test queues
    behind its delay -- the four layer-path launches of case (e) are the longest, the nine library calls and the producer copy of case (a) took
    0.1 ms.  One run out of 36 showed 5.6 ms for the three searches of case (f): host jitter;
  * DELAY_MS = 300 is therefore about 500 times the usual and 50 times the worst host time seen, and well under a second.  The calibration aims 20 %
    above it, and the delay ran 358.9 - 361.2 ms between its two events (torch.cuda.Event pairs) in all 36 test runs.
Every test asserts from its own events that its delay ran at least DELAY_MS (and less than a second) and, by querying the delay's closing event, that
the delay was STILL RUNNING when the last call that has to sit behind it had returned: a delay that was too short fails the test instead of letting
it pass vacuously.

Cases (f) and (g) against the library built from the parent of the commit that added this file (same tests, run once): all three FAIL --
(f) at 8 and at 10 bit: 81.4 % of the nodes of the search queued on stream A came back with a vector or cost that is not the oracle's for
(qp 27, range 33): the third call had rewritten the table for (qp 40, range 24) under it; the two searches on B were right;
(g): the launch queued before fhevc_set_weights came back with logits that are NEITHER blob's (a weight image replaced under a launch whose
parameters were derived from the first blob); the launch after it was right.  The library now waits for the device before it rebuilds the table or touches a weight image."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

from oracle import oracle_py as op
from fasthevc_amd import capi, frames, weights

gpu = pytest.mark.gpu

DELAY_MS = 300.0
CASES = [(416, 240, 8, np.uint8), (416, 240, 10, np.int16), (200, 136, 8, np.uint8), (200, 136, 10, np.int16)]
CASE_IDS = ["416x240-8-uint8", "416x240-10-int16", "200x136-8-uint8", "200x136-10-int16"]
CANARY, COPY_FILL = 0xA5, 0x3C
QP_CNN, MS, MT, QP_FP, QP_MOT, AQ_LAYERS = 30, 3000, 1500, 33, 35, 3
_cache = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def delay_cycles(torch_cuda):
    """cycles for torch.cuda._sleep that last 1.2 * DELAY_MS: the counter's rate is measured here, not assumed"""
    torch = torch_cuda
    assert hasattr(torch.cuda, "_sleep"), "this torch build has no torch.cuda._sleep"
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    probe, ms = 1_000_000, 0.0
    for _ in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 20.0:
            break
        probe *= 4
    assert 20.0 <= ms < 1000.0, f"torch.cuda._sleep({probe}) ran {ms} ms: cannot calibrate the delay"
    cycles = int(probe * 1.2 * DELAY_MS / ms)
    print(f"\n[streams] _sleep({probe}) ran {ms:.1f} ms -> {cycles} cycles for {1.2 * DELAY_MS:.0f} ms")
    return cycles


class _Delay:
    """A spinning kernel on the CURRENT torch stream between two timed events."""

    def __init__(self, torch, cycles):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.e0.record()
        torch.cuda._sleep(cycles)
        self.e1.record()
        self.t0 = time.perf_counter()
        self.host_ms, self.running = None, None

    def issued(self):
        """call when the last host call that has to sit behind the delay has returned"""
        self.running = not self.e1.query()
        self.host_ms = (time.perf_counter() - self.t0) * 1e3

    def check(self, what):
        """after the final synchronise: the delay ran as long as intended and outlasted the host"""
        ms = self.e0.elapsed_time(self.e1)
        print(f"\n[streams] {what}: delay {ms:.1f} ms, host issued the calls behind it in {self.host_ms:.2f} ms")
        assert ms >= DELAY_MS, f"the delay ran only {ms} ms"
        assert ms < 1000.0, f"the delay ran {ms} ms"
        assert self.running, f"the delay was over before the host had issued the calls behind it ({self.host_ms} ms)"


class _Out:
    """nbytes of device output pre-filled with a canary, and the second tensor the consumer copies it to"""

    def __init__(self, torch, nbytes):
        self.t = torch.full((int(nbytes),), CANARY, dtype=torch.uint8, device="cuda")
        self.copy = torch.full((int(nbytes),), COPY_FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()

    def consume(self):
        self.copy.copy_(self.t)

    def result(self, dtype=np.uint8):
        return self.copy.cpu().numpy().view(dtype)


def _on(torch, s):
    return contextlib.nullcontext() if s is None else torch.cuda.stream(s)


# ---- pictures and oracle references (no GPU) --------------------------------------------------------------------------------------------------------------

def _pictures(W, H, bd, seed=0):
    """two pictures of a pan (two overlaid horizontal motions and a vertical one) at bit depth bd, int16, the low bits populated"""
    key = ("pic", W, H, bd, seed)
    if key not in _cache:
        rng = np.random.default_rng(100 * seed + bd)
        ys = frames.pan_clip(max(W, 64), max(H, 64), 2, seed=9 + seed, v_structure=5, v_noise=-3)
        ys = [np.roll(y, 3 * f, axis=0)[:H, :W].astype(np.int16) for f, y in enumerate(ys)]
        _cache[key] = [(y << (bd - 8)) | rng.integers(0, 1 << (bd - 8), size=y.shape).astype(np.int16) for y in ys]
    return _cache[key]


def _poison_pictures(W, H, bd, nf, seed):
    """in-range random samples: what a kernel reads when it runs before its producer (or after the planes were poisoned again)"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, size=(H, W)).astype(np.int16) for _ in range(nf)]


def _valid(W, H, c):
    cw = frames.ctu_grid(W, H)[0]
    return min(64, W - (c % cw) * 64), min(64, H - (c // cw) * 64)


def _classifier_refs(oracle, wkey, w, pics, bd, qp, ms=MS, mt=MT):
    """dict of [nf, ...] arrays: depth, logits, had, flags and the soft ranges at margins (ms, mt)"""
    H, W = pics[0].shape
    key = ("cls", wkey, W, H, bd, qp, ms, mt, tuple(hash(p.tobytes()) for p in pics))
    if key in _cache:
        return _cache[key]
    cw, ch = frames.ctu_grid(W, H)
    n, per = cw * ch, []
    for pic in pics:
        flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
        depth, logits, had = np.zeros(n * 256, np.uint8), np.zeros(n * 42, np.int32), np.zeros(n, np.int32)
        if "widths" in w:
            oracle.fho_predict_frame_family(C.byref(op.family_from_arrays(w)), op.ptr(flat, org), stride, W, H, bd, qp, depth.ctypes.data, logits.ctypes.data)
        else:
            oracle.fho_predict_frame(op.weights_from_arrays(w), op.ptr(flat, org), stride, W, H, bd, qp, depth, C.c_void_p(logits.ctypes.data))
        oracle.fho_frame_src_hadamard(op.ptr(flat, org), stride, W, H, had)
        logits = logits.reshape(n, 42)
        flags = np.zeros(n, np.uint32)
        dmin, dmax = np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint8)
        for c in range(n):
            vw, vh = _valid(W, H, c)
            flags[c] = oracle.fho_flags_from_logits(np.ascontiguousarray(logits[c]), vw, vh)
            oracle.fho_depth_range_from_logits(np.ascontiguousarray(logits[c]), vw, vh, ms, mt, dmin[c], dmax[c])
        per.append(dict(depth=depth.reshape(n, 256), logits=logits, had=had, flags=flags, dmin=dmin, dmax=dmax))
    _cache[key] = {k: np.stack([p[k] for p in per]) for k in per[0]}
    return _cache[key]


def _first_pass_refs(oracle, pics, bd, qp):
    H, W = pics[0].shape
    key = ("fp", W, H, bd, qp)
    if key not in _cache:
        sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
        cw, ch = frames.ctu_grid(W, H)
        out = np.zeros((len(pics), cw * ch, 85), capi.NODE_DTYPE)
        for f, pic in enumerate(pics):
            flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
            for c in range(cw * ch):
                oracle.fho_first_pass_ctu(op.ptr(flat, org), stride, W, H, c % cw, c // cw, bd, sl, out[f, c].ctypes.data_as(C.POINTER(op.NodeCost)))
        _cache[key] = out
    return _cache[key]


def _preanalyze_refs(oracle, pics, bd, layers):
    H, W = pics[0].shape
    key = ("aq", W, H, bd, layers)
    if key not in _cache:
        out = []
        for pic in pics:
            flat, org, stride, _ = frames.guarded_plane(pic, bd, poison=None)
            acts = []
            for d in range(layers):
                p = 64 >> d
                a = np.zeros(((H + p - 1) // p) * ((W + p - 1) // p))
                oracle.fho_preanalyze_layer(op.ptr(flat, org), stride, W, H, p, a)
                acts.append(a)
            out.append(np.concatenate(acts))
        _cache[key] = np.stack(out)
    return _cache[key]


def _motion_refs(oracle, pair, bd, qp, rng, sad, ctus=None, tag=""):
    """[numCtus, 85] nodes of pair[1] searched in pair[0] (fho_motion_ctu_dist); CTUs outside `ctus` stay zero"""
    H, W = pair[0].shape
    cw, ch = frames.ctu_grid(W, H)
    ctus = list(range(cw * ch)) if ctus is None else list(ctus)
    key = ("mot", tag, W, H, bd, qp, rng, sad, tuple(ctus))
    if key not in _cache:
        flat, org, stride, fs = frames.guarded_plane(list(pair), bd, poison=None)
        sl = oracle.fho_lambda_intra(qp, bd) ** 0.5
        out = np.zeros((cw * ch, 85), capi.MOTION_DTYPE)
        for c in ctus:
            oracle.fho_motion_ctu_dist(op.ptr(flat, org + fs), stride, op.ptr(flat, org), stride, W, H, c % cw, c // cw, bd, rng, C.c_double(sl), int(sad),
                                       C.c_void_p(out[c].ctypes.data))
        _cache[key] = out
    return _cache[key]


def _differing_nodes(a, b):
    """share of the nodes inside the picture whose vector or cost differs between two searches of the same picture pair"""
    valid = a["cost_best"] != 0xFFFFFFFF
    assert np.array_equal(valid, b["cost_best"] != 0xFFFFFFFF) and valid.sum() > 0
    diff = (a["cost_best"] != b["cost_best"]) | (a["mvx"] != b["mvx"]) | (a["mvy"] != b["mvy"])
    return float((diff & valid).sum()) / float(valid.sum())


def _same_nodes(got, exp, dtype=capi.MOTION_DTYPE):
    return [k for k in dtype.names if not np.array_equal(got[k], exp[k])]


# ---- the oracle-only preconditions of (f) and (g): they run without a GPU ---------------------------------------------------------------------------------

WIDE = dict(W=416, H=240, qp_a=27, rng_a=33, qp_b=40, rng_b=24)


def _wide_pairs(bd):
    """A's pair: a noisy picture (the noise of every second 16x16 block has sigma 18) panning 21 samples against a structure moving 13 the other
    way -- most nodes win with a long vector, whose cost (and, where two candidates are close, whose choice) depends on the QP; B's pair: another clip"""
    key = ("widepairs", bd)
    if key not in _cache:
        out = []
        for seed, vs, vn in ((3, -13, 21), (4, 9, -17)):
            rng = np.random.default_rng(10 * seed + bd)
            ys = frames.pan_clip(WIDE["W"], WIDE["H"], 2, seed=seed, v_structure=vs, v_noise=vn)
            out.append([(y.astype(np.int16) << (bd - 8)) | rng.integers(0, 1 << (bd - 8), size=y.shape).astype(np.int16) for y in ys])
        _cache[key] = out
    return _cache[key]


def _wide_case(oracle, bd):
    """references of case (f) and its precondition: on A's pair the two settings differ in at least a tenth of the nodes inside the picture"""
    pa, pb = _wide_pairs(bd)
    cw = frames.ctu_grid(WIDE["W"], WIDE["H"])[0]
    ref_a = _motion_refs(oracle, pa, bd, WIDE["qp_a"], WIDE["rng_a"], True, tag="wideA")
    other = _motion_refs(oracle, pa, bd, WIDE["qp_b"], WIDE["rng_a"], True, tag="wideA")
    share = _differing_nodes(ref_a, other)
    assert share >= 0.1, f"qp {WIDE['qp_a']} and {WIDE['qp_b']} differ in only {share:.3f} of the nodes: the case proves nothing"
    row0 = range(cw)
    ref_b1 = _motion_refs(oracle, pb, bd, WIDE["qp_a"], WIDE["rng_a"], True, ctus=row0, tag="wideB")[:cw]
    ref_b2 = _motion_refs(oracle, pb, bd, WIDE["qp_b"], WIDE["rng_b"], True, ctus=row0, tag="wideB")[:cw]
    return pa, pb, ref_a, ref_b1, ref_b2, share


BLOB = dict(W=416, H=240, bd=8, qp=32)


def _blob_case(oracle):
    """references of case (g) and its precondition: the two blobs give different logits (and depth maps) on the picture"""
    w1, w2 = weights.random_weights(1), weights.random_weights(2)
    pics = _pictures(BLOB["W"], BLOB["H"], BLOB["bd"])[:1]
    r1 = _classifier_refs(oracle, "base1", w1, pics, BLOB["bd"], BLOB["qp"])
    r2 = _classifier_refs(oracle, "base2", w2, pics, BLOB["bd"], BLOB["qp"])
    ctus = (r1["logits"] != r2["logits"]).any(axis=-1)
    assert ctus.all(), "the two blobs give the same logits on some CTU: the case proves nothing"
    assert not np.array_equal(r1["depth"], r2["depth"])
    return w1, w2, pics, r1, r2


@pytest.mark.parametrize("bd", [8, 10])
def test_f_precondition_the_two_cost_tables_give_different_searches(oracle, bd):
    share = _wide_case(oracle, bd)[-1]
    print(f"\n[streams] wide search at {bd} bit: qp 27 and qp 40 differ in {share:.3f} of the nodes inside the picture")


def test_g_precondition_the_two_blobs_give_different_logits(oracle):
    _blob_case(oracle)


# ---- (a), (b), (c): producer / library / consumer chains behind a delay -----------------------------------------------------------------------------------

class _Chain:
    """Device buffers of one case: the planes (poison now, the real pictures in a staging tensor), and one _Out per result."""

    def __init__(self, torch, W, H, bd, dtype, seed=0):
        self.torch, self.W, self.H, self.bd = torch, W, H, bd
        self.pics = _pictures(W, H, bd)
        nf = len(self.pics)
        real, org, stride, fs = frames.guarded_plane(self.pics, bd, dtype, poison=11 + seed)
        bad = [frames.guarded_plane(_poison_pictures(W, H, bd, nf, 21 + seed + k), bd, dtype, poison=31 + seed + k)[0] for k in range(2)]
        assert all(b.shape == real.shape for b in bad) and not np.array_equal(bad[0], real)
        self.item, self.org, self.stride, self.fs, self.nf = np.dtype(dtype).itemsize, org, stride, fs, nf
        self.staging = torch.from_numpy(real).cuda()
        self.poison_after = torch.from_numpy(bad[1]).cuda()
        self.planes = torch.from_numpy(bad[0]).cuda()          # what the library is given: poison until the producer has run
        self.warm = torch.from_numpy(real).cuda()               # a second copy of the real planes for the warm-up launches
        self.ptr = self.planes.data_ptr() + self.item * org
        self.warm_ptr = self.warm.data_ptr() + self.item * org
        self.outs = {}

    def out(self, name, nbytes):
        self.outs[name] = _Out(self.torch, nbytes)
        return self.outs[name].ptr

    def produce(self):
        self.planes.copy_(self.staging)

    def consume_and_poison(self):
        for o in self.outs.values():
            o.consume()
        self.planes.copy_(self.poison_after)


def _classifier_calls(ctx, ch, ptr, stream, scratch=False):
    """the classifier's three entry points; expand reads the flag words the first call writes (ordered on the same stream)"""
    n, nf = ctx.num_ctus, ch.nf
    names = ("depth", "had", "logits", "flags", "dmin", "dmax", "had_r", "logits_r", "flags_r", "expanded")
    sizes = (nf * n * 256, nf * n * 4, nf * n * 42 * 4, nf * n * 4, nf * n * 256, nf * n * 256, nf * n * 4, nf * n * 42 * 4, nf * n * 4, nf * n * 256)
    if scratch:
        p = {k: _Out(ch.torch, s) for k, s in zip(names, sizes)}
        ch.scratch = getattr(ch, "scratch", []) + [p]
        p = {k: v.ptr for k, v in p.items()}
    else:
        p = {k: ch.out(k, s) for k, s in zip(names, sizes)}
    a = (ptr, ch.item, ch.stride, ch.fs, nf)
    return [lambda: ctx.predict_frames_device(*a, p["depth"], p["had"], p["logits"], stream=stream, qp=QP_CNN, d_flags=p["flags"]),
            lambda: ctx.predict_frames_device_range(*a, p["dmin"], p["dmax"], p["had_r"], p["logits_r"], stream=stream, qp=QP_CNN, d_flags=p["flags_r"],
                                                    margin_split=MS, margin_stop=MT),
            lambda: ctx.expand_depth_flags_device(p["flags"], nf, p["expanded"], stream=stream)]


def _check_classifier(oracle, ctx, ch, w, wkey, what):
    n, nf = ctx.num_ctus, ch.nf
    ref = _classifier_refs(oracle, wkey, w, ch.pics, ch.bd, QP_CNN)
    o = ch.outs
    got = dict(depth=o["depth"].result().reshape(nf, n, 256), had=o["had"].result(np.int32).reshape(nf, n), logits=o["logits"].result(np.int32).reshape(nf, n, 42),
               flags=o["flags"].result(np.uint32).reshape(nf, n), dmin=o["dmin"].result().reshape(nf, n, 256), dmax=o["dmax"].result().reshape(nf, n, 256),
               had_r=o["had_r"].result(np.int32).reshape(nf, n), logits_r=o["logits_r"].result(np.int32).reshape(nf, n, 42),
               expanded=o["expanded"].result().reshape(nf, n, 256))
    for k, v in got.items():
        exp = ref[{"had_r": "had", "logits_r": "logits", "expanded": "depth"}.get(k, k)]
        bad = np.argwhere(v != exp)
        assert bad.size == 0, (what, k, "first differences [frame, CTU, ...]:", bad[:4].tolist())
    assert len(np.unique(ref["depth"])) >= 2


def _other_calls(ctx, ch, ptr, stream, scratch=False):
    """first pass, AQ pre-analysis, the small SATD search and the wide SAD search (the distortion is switched between the two launches)"""
    n, nf = ctx.num_ctus, ch.nf
    total = ctx.aq_layout(AQ_LAYERS)[-1]
    names, sizes = ("nodes", "act", "mot4", "mot33"), (nf * n * 85 * 16, nf * total * 8, (nf - 1) * n * 85 * 16, (nf - 1) * n * 85 * 16)
    if scratch:
        p = {k: _Out(ch.torch, s) for k, s in zip(names, sizes)}
        ch.scratch = getattr(ch, "scratch", []) + [p]
        p = {k: v.ptr for k, v in p.items()}
    else:
        p = {k: ch.out(k, s) for k, s in zip(names, sizes)}
    a = (ptr, ch.item, ch.stride, ch.fs, nf)
    return [lambda: ctx.intra_first_pass_device(*a, p["nodes"], stream=stream, qp=QP_FP),
            lambda: ctx.preanalyze_frames_device(*a, p["act"], max_aq_depth=AQ_LAYERS, stream=stream),
            lambda: ctx.set_motion_distortion("satd"),
            lambda: ctx.motion_search_device(*a, p["mot4"], stream=stream, qp=QP_MOT, search_range=4),
            lambda: ctx.set_motion_distortion("sad"),
            lambda: ctx.motion_search_device(*a, p["mot33"], stream=stream, qp=QP_MOT, search_range=33)]


def _check_other(oracle, ctx, ch, what):
    n, nf, o = ctx.num_ctus, ch.nf, ch.outs
    nodes = o["nodes"].result(capi.NODE_DTYPE).reshape(nf, n, 85)
    assert _same_nodes(nodes, _first_pass_refs(oracle, ch.pics, ch.bd, QP_FP), capi.NODE_DTYPE) == [], (what, "first pass")
    act = o["act"].result(np.float64).reshape(nf, -1)
    assert act.tobytes() == _preanalyze_refs(oracle, ch.pics, ch.bd, AQ_LAYERS).tobytes(), (what, "pre-analysis")
    mot4 = o["mot4"].result(capi.MOTION_DTYPE).reshape(n, 85)
    assert _same_nodes(mot4, _motion_refs(oracle, ch.pics, ch.bd, QP_MOT, 4, False)) == [], (what, "motion search, range 4, SATD")
    mot33 = o["mot33"].result(capi.MOTION_DTYPE).reshape(n, 85)
    assert _same_nodes(mot33, _motion_refs(oracle, ch.pics, ch.bd, QP_MOT, 33, True)) == [], (what, "motion search, range 33, SAD")


def _run_chain(torch, ch, stream, cycles, warm, calls, what, expect_async):
    """warm-up on scratch buffers (code objects, the cost table, lazy allocations), then: delay | producer | library | consumer | poison"""
    for f in warm:
        f()
    torch.cuda.synchronize()
    pending = []
    with _on(torch, stream):
        delay = _Delay(torch, cycles)
        ch.produce()
        for f in calls:
            f()
            if expect_async:   # (c): the call has returned; nothing of it can have run, the delay in front of it is still spinning
                ev = torch.cuda.Event()
                ev.record()
                pending.append((ev.query(), delay.e1.query()))
        delay.issued()
        ch.consume_and_poison()
    torch.cuda.synchronize()
    delay.check(what)
    for done, delay_over in pending:
        assert not delay_over, (what, "the delay was over while the calls were being issued")
        assert done is False, (what, "an event behind the call was complete while the delay before it was still running")


@gpu
@pytest.mark.parametrize("W,H,bd,dtype", CASES, ids=CASE_IDS)
def test_a_default_stream_caller_needs_no_synchronisation(oracle, torch_cuda, delay_cycles, W, H, bd, dtype):
    """(a) everything on torch's default stream (the legacy stream 0), the library with stream = NULL, one synchronise at the very end: the library
    waited for the producer queued before it, and the consumer queued after it waited for the library -- both halves of the header's sentence"""
    torch, w = torch_cuda, weights.random_weights(6)
    ctx = capi.Context(W, H, bd, w, max_frames=2)
    ch = _Chain(torch, W, H, bd, dtype)
    warm = _classifier_calls(ctx, ch, ch.warm_ptr, None, scratch=True) + _other_calls(ctx, ch, ch.warm_ptr, None, scratch=True)
    calls = _classifier_calls(ctx, ch, ch.ptr, None) + _other_calls(ctx, ch, ch.ptr, None)
    what = ("default stream", W, H, bd, dtype.__name__)
    _run_chain(torch, ch, None, delay_cycles, warm, calls, what, expect_async=False)
    _check_classifier(oracle, ctx, ch, w, "base6", what)
    _check_other(oracle, ctx, ch, what)
    ctx.close()


@gpu
@pytest.mark.parametrize("W,H,bd,dtype", CASES, ids=CASE_IDS)
def test_b_c_caller_stream_classifier(oracle, torch_cuda, delay_cycles, cnn_arith, W, H, bd, dtype):
    """(b) the same chain on a caller's non-blocking stream, which the library is given; the default stream and the context's own stream stay idle, so a
    library that launched there would read poison.  (c) an event recorded behind each call is not complete while the delay is running.
    Every launch shape of the classifier (cnn_arith)."""
    torch, w = torch_cuda, weights.random_weights(6)
    s = torch.cuda.Stream()
    ctx = capi.Context(W, H, bd, w, max_frames=2)
    ch = _Chain(torch, W, H, bd, dtype, seed=1)
    what = ("caller stream", cnn_arith, W, H, bd, dtype.__name__)
    _run_chain(torch, ch, s, delay_cycles, _classifier_calls(ctx, ch, ch.warm_ptr, s.cuda_stream, scratch=True), _classifier_calls(ctx, ch, ch.ptr, s.cuda_stream), what,
               expect_async=True)
    _check_classifier(oracle, ctx, ch, w, "base6", what)
    ctx.close()


@gpu
@pytest.mark.parametrize("W,H,bd,dtype", CASES, ids=CASE_IDS)
def test_b_c_caller_stream_first_pass_preanalysis_motion(oracle, torch_cuda, delay_cycles, W, H, bd, dtype):
    """(b), (c) for fhevc_intra_first_pass_device, fhevc_preanalyze_frames_device and fhevc_motion_search_device (range 4 SATD, range 33 SAD)"""
    torch = torch_cuda
    s = torch.cuda.Stream()
    ctx = capi.Context(W, H, bd, max_frames=2)
    ch = _Chain(torch, W, H, bd, dtype, seed=2)
    what = ("caller stream", W, H, bd, dtype.__name__)
    _run_chain(torch, ch, s, delay_cycles, _other_calls(ctx, ch, ch.warm_ptr, s.cuda_stream, scratch=True), _other_calls(ctx, ch, ch.ptr, s.cuda_stream), what, expect_async=True)
    _check_other(oracle, ctx, ch, what)
    ctx.close()


# ---- (d): settings take effect at the next launch ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("first", ["i8", "f16"])
def test_d_cnn_arith_switches_at_the_next_launch(oracle, torch_cuda, delay_cycles, first):
    """a launch queued in one arithmetic form, fhevc_set_cnn_arith at once, a second launch in the other form: both deliver the oracle's integers (both
    forms do, so this guards against a switch that tears the queued launch, not against a value change)"""
    torch, W, H, bd = torch_cuda, 416, 240, 8
    w, other = weights.random_weights(6), {"i8": "f16", "f16": "i8"}[first]
    pics = _pictures(W, H, bd)
    ref = _classifier_refs(oracle, "base6", w, pics, bd, QP_CNN)
    flat, org, stride, fs = frames.guarded_plane(pics, bd, np.uint8, poison=5)
    ctx = capi.Context(W, H, bd, w, max_frames=2, arith=first)
    n, s = ctx.num_ctus, torch.cuda.Stream()
    planes = torch.from_numpy(flat).cuda()
    outs = [{k: _Out(torch, 2 * n * b) for k, b in (("depth", 256), ("had", 4), ("logits", 168), ("flags", 4))} for _ in range(3)]

    def call(o):
        ctx.predict_frames_device(planes.data_ptr() + org, 1, stride, fs, 2, o["depth"].ptr, o["had"].ptr, o["logits"].ptr, stream=s.cuda_stream, qp=QP_CNN,
                                  d_flags=o["flags"].ptr)
    for a in (other, first):   # warm-up of both forms; ends in `first`
        ctx.set_cnn_arith(a)
        call(outs[2])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay = _Delay(torch, delay_cycles)
        call(outs[0])
        ctx.set_cnn_arith(other)
        call(outs[1])
        delay.issued()
        for o in outs[:2]:
            for v in o.values():
                v.consume()
    torch.cuda.synchronize()
    delay.check(("cnn_arith", first))
    assert ctx.cnn_arith == other
    for i, o in enumerate(outs[:2]):
        assert np.array_equal(o["depth"].result().reshape(2, n, 256), ref["depth"]), (first, i)
        assert np.array_equal(o["logits"].result(np.int32).reshape(2, n, 42), ref["logits"]), (first, i)
        assert np.array_equal(o["had"].result(np.int32).reshape(2, n), ref["had"]), (first, i)
        assert np.array_equal(o["flags"].result(np.uint32).reshape(2, n), ref["flags"]), (first, i)
    ctx.close()


@gpu
@pytest.mark.parametrize("bd,dtype", [(8, np.uint8), (10, np.int16)], ids=["8-uint8", "10-int16"])
def test_d_motion_distortion_switches_at_the_next_launch(oracle, torch_cuda, delay_cycles, bd, dtype):
    """two small-range searches with fhevc_set_motion_distortion between them: the first comes back as SATD, the second as SAD"""
    torch, W, H, rng = torch_cuda, 416, 240, 4
    pics = _pictures(W, H, bd)
    ref_satd, ref_sad = _motion_refs(oracle, pics, bd, QP_MOT, rng, False), _motion_refs(oracle, pics, bd, QP_MOT, rng, True)
    assert _same_nodes(ref_satd, ref_sad) != []
    flat, org, stride, fs = frames.guarded_plane(pics, bd, dtype, poison=6)
    item = np.dtype(dtype).itemsize
    ctx = capi.Context(W, H, bd, max_frames=2)
    n, s = ctx.num_ctus, torch.cuda.Stream()
    planes = torch.from_numpy(flat).cuda()
    outs = [_Out(torch, n * 85 * 16) for _ in range(3)]

    def call(o):
        ctx.motion_search_device(planes.data_ptr() + item * org, item, stride, fs, 2, o.ptr, stream=s.cuda_stream, qp=QP_MOT, search_range=rng)
    for m in ("sad", "satd"):
        ctx.set_motion_distortion(m)
        call(outs[2])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay = _Delay(torch, delay_cycles)
        call(outs[0])
        ctx.set_motion_distortion("sad")
        call(outs[1])
        delay.issued()
        outs[0].consume()
        outs[1].consume()
    torch.cuda.synchronize()
    delay.check(("motion distortion", bd))
    assert _same_nodes(outs[0].result(capi.MOTION_DTYPE).reshape(n, 85), ref_satd) == [], "the launch queued before the switch"
    assert _same_nodes(outs[1].result(capi.MOTION_DTYPE).reshape(n, 85), ref_sad) == [], "the launch queued after the switch"
    ctx.close()


# ---- (e): the layer path's activation tensors, shared by two streams --------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("heads", ["delay-on-A", "delay-on-A-and-B"])
def test_e_layer_path_on_two_streams(oracle, torch_cuda, delay_cycles, monkeypatch, heads):
    """A member that runs layer by layer through HBM keeps ONE set of activation tensors per context.  Streams A and B, different pictures on each, calls
    issued A, B, A, B without host synchronisation: each launch has to wait (lw_done) for the one before it on the other stream.  With the delay at the
    head of A only, B's first launch must wait for A's behind the delay; with the same delay at the head of both, the two streams become free at the
    same moment, so launches that did not wait for each other would run on the shared tensors at once."""
    torch, W, H, bd, qp = torch_cuda, 416, 240, 8, 27
    monkeypatch.setenv("FHEVC_FAMILY_LAYERS", "1")
    fam = weights.random_family((18, 36, 72), 3, seed=1)
    pics = _pictures(W, H, bd, seed=1)
    ref = _classifier_refs(oracle, "fam18x3", fam, pics, bd, qp)
    ctx = capi.Context(W, H, bd, fam, max_frames=1)
    n = ctx.num_ctus
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    planes = []
    for p in pics:
        flat, org, stride, _ = frames.guarded_plane(p, bd, np.uint8, poison=7)
        planes.append((torch.from_numpy(flat).cuda(), org, stride))
    order = [(A, 0), (B, 1), (A, 1), (B, 0)]
    outs = [{k: _Out(torch, n * b) for k, b in (("depth", 256), ("logits", 168), ("flags", 4))} for _ in range(len(order) + 1)]

    def call(s, pic, o):
        t, org, stride = planes[pic]
        ctx.predict_frames_device(t.data_ptr() + org, 1, stride, 0, 1, o["depth"].ptr, None, o["logits"].ptr, stream=s.cuda_stream, qp=qp, d_flags=o["flags"].ptr)
    call(A, 0, outs[-1])
    torch.cuda.synchronize()
    delays = []
    for s in ([A] if heads == "delay-on-A" else [A, B]):
        with torch.cuda.stream(s):
            delays.append(_Delay(torch, delay_cycles))
    for (s, pic), o in zip(order, outs):
        call(s, pic, o)
    for d in delays:
        d.issued()
    for (s, _), o in zip(order, outs):
        with torch.cuda.stream(s):
            for v in o.values():
                v.consume()
    torch.cuda.synchronize()
    for d in delays:
        d.check(("layer path", heads))
    for i, ((_, pic), o) in enumerate(zip(order, outs)):
        assert np.array_equal(o["logits"].result(np.int32).reshape(n, 42), ref["logits"][pic]), (heads, "call", i)
        assert np.array_equal(o["depth"].result().reshape(n, 256), ref["depth"][pic]), (heads, "call", i)
        assert np.array_equal(o["flags"].result(np.uint32), ref["flags"][pic]), (heads, "call", i)
    assert not np.array_equal(ref["logits"][0], ref["logits"][1])
    ctx.close()


# ---- (f): the vector-cost table of the wide search, two streams -------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("bd,dtype", [(8, np.uint8), (10, np.int16)], ids=["8-uint8", "10-int16"])
def test_f_wide_cost_table_is_rebuilt_behind_every_reader(oracle, torch_cuda, delay_cycles, bd, dtype):
    """One table of vector costs per context (k_motion_wide.hip at 8 bit, fhevc_launch_motion_big above).  A wide search (qp 27, range 33) queued on
    stream A behind a delay, a second with the same setting on stream B, then one with (qp 40, range 24) on B, which rebuilds the table: the rebuild has
    to wait for A's launch too, not only for the latest reader."""
    torch, W, H = torch_cuda, WIDE["W"], WIDE["H"]
    pa, pb, ref_a, ref_b1, ref_b2, _ = _wide_case(oracle, bd)
    item = np.dtype(dtype).itemsize
    ctx = capi.Context(W, H, bd, max_frames=2)
    ctx.set_motion_distortion("sad")
    n, cw = ctx.num_ctus, ctx.ctus_x
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    dev = []
    for pair in (pa, pb):
        flat, org, stride, fs = frames.guarded_plane(pair, bd, dtype, poison=8)
        t = torch.from_numpy(flat).cuda()
        dev.append((t, t.data_ptr() + item * org, stride, fs))
    out_a, out_b1, out_b2, scratch = _Out(torch, n * 85 * 16), _Out(torch, cw * 85 * 16), _Out(torch, cw * 85 * 16), _Out(torch, n * 85 * 16)

    def search(which, s, o, qp, rng, rows=None):
        _, ptr, stride, fs = dev[which]
        ctx.motion_search_device(ptr, item, stride, fs, 2, o.ptr, rows=rows, stream=s.cuda_stream, qp=qp, search_range=rng)
    search(0, A, scratch, WIDE["qp_a"], WIDE["rng_a"])   # warm-up: the kernel's code object and the table for (qp 27, range 33)
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        delay = _Delay(torch, delay_cycles)
    search(0, A, out_a, WIDE["qp_a"], WIDE["rng_a"])
    search(1, B, out_b1, WIDE["qp_a"], WIDE["rng_a"], rows=(0, 1))
    delay.issued()
    search(1, B, out_b2, WIDE["qp_b"], WIDE["rng_b"], rows=(0, 1))
    with torch.cuda.stream(A):
        out_a.consume()
    with torch.cuda.stream(B):
        out_b1.consume()
        out_b2.consume()
    torch.cuda.synchronize()
    delay.check(("wide table", bd))
    got_a = out_a.result(capi.MOTION_DTYPE).reshape(n, 85)
    bad = _same_nodes(got_a, ref_a)
    if bad:
        wrong = float(((got_a["cost_best"] != ref_a["cost_best"]) | (got_a["mvx"] != ref_a["mvx"]) | (got_a["mvy"] != ref_a["mvy"])).mean())
        print(f"\n[streams] wide table, {bd} bit: {wrong:.3f} of the nodes of A's search differ from the oracle at (qp 27, range 33)")
    assert bad == [], ("the search queued on A before the rebuild", bad)
    assert _same_nodes(out_b1.result(capi.MOTION_DTYPE).reshape(cw, 85), ref_b1) == [], "the second search (B, same setting)"
    assert _same_nodes(out_b2.result(capi.MOTION_DTYPE).reshape(cw, 85), ref_b2) == [], "the third search (B, rebuilt table)"
    ctx.close()


# ---- (g): fhevc_set_weights under queued work -------------------------------------------------------------------------------------------------------------

@gpu
def test_g_set_weights_under_queued_work(oracle, torch_cuda, delay_cycles):
    """FHW1 over FHW1 (overwritten in place, nothing is freed): a launch queued on a caller's stream with blob 1 loaded, fhevc_set_weights(blob 2) at once,
    a second launch: the first delivers the oracle's results for blob 1, the second those for blob 2"""
    torch, W, H, bd, qp = torch_cuda, BLOB["W"], BLOB["H"], BLOB["bd"], BLOB["qp"]
    w1, w2, pics, r1, r2 = _blob_case(oracle)
    flat, org, stride, _ = frames.guarded_plane(pics[0], bd, np.uint8, poison=9)
    ctx = capi.Context(W, H, bd, w1)
    n, s = ctx.num_ctus, torch.cuda.Stream()
    planes = torch.from_numpy(flat).cuda()
    outs = [{k: _Out(torch, n * b) for k, b in (("depth", 256), ("had", 4), ("logits", 168))} for _ in range(3)]

    def call(o):
        ctx.predict_frames_device(planes.data_ptr() + org, 1, stride, 0, 1, o["depth"].ptr, o["had"].ptr, o["logits"].ptr, stream=s.cuda_stream, qp=qp)
    call(outs[2])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay = _Delay(torch, delay_cycles)
    call(outs[0])
    delay.issued()
    ctx.set_weights(w2)
    call(outs[1])
    with torch.cuda.stream(s):
        for o in outs[:2]:
            for v in o.values():
                v.consume()
    torch.cuda.synchronize()
    delay.check("set_weights")
    for i, (o, ref) in enumerate(zip(outs[:2], (r1, r2))):
        got = o["logits"].result(np.int32).reshape(n, 42)
        if not np.array_equal(got, ref["logits"][0]):
            print(f"\n[streams] set_weights: launch {i} equals blob 1: {np.array_equal(got, r1['logits'][0])}, blob 2: {np.array_equal(got, r2['logits'][0])}")
        assert np.array_equal(got, ref["logits"][0]), ("logits of launch", i, "do not belong to blob", i + 1)
        assert np.array_equal(o["depth"].result().reshape(n, 256), ref["depth"][0]), ("depth maps of launch", i)
        assert np.array_equal(o["had"].result(np.int32), ref["had"][0]), ("source Hadamard of launch", i)
    ctx.close()
