"""Config 4 (P slices): what every host form of the motion entry points moves besides its results -- the bytes it counts up and down, the launches
it counts, and nothing at all when it rejects its arguments.  The results themselves are pinned by the tests of each stage; here the expected figures are
sums of 2 * W * H * 2 (the staged pair), numCtus * {1, 85, 124, 384} * 16 (centres, nodes, PUs, small PUs), numCtus * 256 (a depth map) and the number of
launches read off the entry point's branches.

The picture is 136 x 72 = 3 x 2 CTUs, ragged on both sides: numCtus = 6, so no family's size is a power of two.  The planes lie inside a larger array at
a non-zero origin with a stride above the width.  FHEVC_HOST_FORMS_LIB names another build of the library (tools/build_variant.sh) to run the same
checks against, e.g. the commit before a change to the C-ABI layer."""
import itertools
import os

import numpy as np
import pytest

from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, clip_planes

pytestmark = pytest.mark.gpu

W, H, N = 136, 72, 6
STRIDE, TOP, LEFT = W + 11, 4, 3
ORG = TOP * STRIDE + LEFT
QP = 30
PAIR = 2 * W * H * 2
MAPS = N * 256
NODES, PUS, SMALL = capi.NODES_PER_CTU, capi.PUS_PER_CTU, capi.PUS_SMALL_PER_CTU
FAMILIES = (NODES, PUS, SMALL)
COMBOS = [c for c in itertools.product((True, False), repeat=3) if any(c)]
COUNTERS = ("bytes_h2d", "bytes_d2h", "kernels_launched")


def F(per_ctu):
    return N * per_ctu * 16


def asked(combo):
    return sum(F(k) for k, want in zip(FAMILIES, combo) if want)


def pick(arrays, combo):
    return dict(zip(("nodes", "pus", "pus_small"), (a if want else None for a, want in zip(arrays, combo))))


def embed(pic):
    buf = np.full((H + 9, STRIDE), 77, np.int16)
    buf[TOP:TOP + H, LEFT:LEFT + W] = pic
    return buf


class World:
    """one context and one picture pair of a bit depth, and the inputs the refinements and the merge stage take, from the searches of the same pair"""

    def __init__(self, bd, sad=False):
        self.ctx = capi.Context(W, H, bd, lib_path=os.environ.get("FHEVC_HOST_FORMS_LIB"))
        assert self.ctx.num_ctus == N
        if sad:
            self.ctx.set_motion_distortion("sad")
        ref, cur = clip_planes(frames.pan_clip(W, H, 2, seed=40 + bd, v_structure=3, v_noise=-2), bd, low_bits_seed=3)
        self.cur, self.ref = embed(cur), embed(ref)
        self.at = dict(origin=ORG, stride=STRIDE, qp=QP)

    def counted(self, call):
        before = self.ctx.stats()
        res = call()
        after = self.ctx.stats()
        return res, tuple(after[k] - before[k] for k in COUNTERS)

    def found(self, R):
        return self.ctx.motion_search_pu_wide(self.cur, self.ref, search_range=R, **self.at)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def w8():
    w = World(8)
    yield w
    w.close()


@pytest.fixture(scope="module")
def w8_sad():
    w = World(8, sad=True)
    yield w
    w.close()


@pytest.fixture(scope="module")
def w10():
    w = World(10)
    yield w
    w.close()


# ---- 1. the counters of accepted calls -----------------------------------------------------------------------------------------------------------------------

def test_counters_of_the_forms_with_one_output(w8, w8_sad):
    for w, R in ((w8, 4), (w8_sad, 4), (w8_sad, 9)):       # above 8 the search takes the SAD distortion
        c, cur, ref, at = w.ctx, w.cur, w.ref, w.at
        assert w.counted(lambda: c.motion_search(cur, ref, search_range=R, **at))[1] == (PAIR, F(NODES), 1), R
        nodes = w.found(R)[0]
        refined, d = w.counted(lambda: c.motion_refine(cur, ref, nodes, max_range=R, **at))
        assert d == (PAIR + F(NODES), F(NODES), 1), R
        assert w.counted(lambda: c.motion_merge(cur, ref, refined, max_range=R, **at))[1] == (PAIR + F(NODES), F(NODES), 1), R
    c, cur, ref, at = w8.ctx, w8.cur, w8.ref, w8.at
    for R in (1, 8):
        assert w8.counted(lambda: c.motion_search_pu(cur, ref, search_range=R, **at))[1] == (PAIR, F(PUS), 1), R
        assert w8.counted(lambda: c.motion_search_pu(cur, ref, search_range=R, with_nodes=True, **at))[1] == (PAIR, F(PUS) + F(NODES), 1), R
        assert w8.counted(lambda: c.motion_search_pu_small(cur, ref, search_range=R, **at))[1] == (PAIR, F(SMALL), 1), R
    for coarse in (1, 14):
        assert w8.counted(lambda: c.motion_centres(cur, ref, coarse_range=coarse, **at))[1] == (PAIR, F(1), 1), coarse


@pytest.mark.parametrize("combo", COMBOS)
def test_counters_of_the_forms_with_optional_families(w8, w10, combo):
    nodes, pus, small = combo
    two = int(nodes or pus) + int(small)           # the generic searches: one launch for nodes and PUs, one for the small PUs
    pairs = int(nodes) + int(pus or small)         # the refinements: one launch for the nodes, one for both PU families
    c, cur, ref, at = w8.ctx, w8.cur, w8.ref, w8.at
    want = dict(nodes=nodes, pus=pus, pus_small=small)
    # the wide search: up to +-8 the generic kernels; above, 8-bit contexts take the byte-SAD kernel (one launch for whatever is asked for) and
    # contexts above 8 bit the generic kernels again
    assert w8.counted(lambda: c.motion_search_pu_wide(cur, ref, search_range=8, **want, **at))[1] == (PAIR, asked(combo), two)
    assert w8.counted(lambda: c.motion_search_pu_wide(cur, ref, search_range=9, **want, **at))[1] == (PAIR, asked(combo), 1)
    assert w10.counted(lambda: w10.ctx.motion_search_pu_wide(w10.cur, w10.ref, search_range=9, **want, **w10.at))[1] == (PAIR, asked(combo), two)
    for R in (8, 9):
        ins = pick(w8.found(R), combo)
        assert w8.counted(lambda: c.motion_refine_pu_wide(cur, ref, max_range=R, **ins, **at))[1] == (PAIR + asked(combo), asked(combo), pairs), R
    ins = pick(w10.found(9), combo)
    assert w10.counted(lambda: w10.ctx.motion_refine_pu_wide(w10.cur, w10.ref, max_range=9, **ins, **w10.at))[1] == (PAIR + asked(combo), asked(combo), pairs)
    if pus or small:
        found = w8.found(4)
        for R in (4, 8):
            ins = dict(pus=found[1] if pus else None, pus_small=found[2] if small else None)
            assert w8.counted(lambda: c.motion_refine_pu(cur, ref, max_range=R, **ins, **at))[1] == (PAIR + asked((False, pus, small)), asked((False, pus, small)), 1), R
    # around one centre per CTU: the centres go up beside the pair
    centres = c.motion_centres(cur, ref, coarse_range=5, **at)
    for R in (3, 8):
        got, d = w8.counted(lambda: c.motion_search_pu_centred(cur, ref, centres, search_range=R, **want, **at))
        assert d == (PAIR + F(1), asked(combo), two), R
        ins = pick(got, combo)
        assert w8.counted(lambda: c.motion_refine_pu_centred(cur, ref, centres, max_range=R, **ins, **at))[1] == (PAIR + F(1) + asked(combo), asked(combo), pairs), R


def test_counters_of_the_frame_calls(w8, w8_sad, w10):
    prev = np.random.default_rng(5).integers(0, 4, size=(N, 256)).astype(np.uint8)
    for w, R in ((w8, 4), (w8_sad, 9)):
        assert w.counted(lambda: w.ctx.p_predict_frame(w.cur, w.ref, prev, search_range=R, **w.at))[1] == (PAIR + MAPS, 2 * MAPS, 2), R
    # the chains: the wide search (two launches up to +-8; above, one at 8 bit and two above 8 bit), its refinement (two), then one launch per stage;
    # around coarse centres: their launch, two of the centred search, two of the centred refinement
    for w, R, coarse, search in ((w8, 8, 0, 2), (w8, 9, 0, 1), (w10, 9, 0, 2), (w8, 8, 5, 3), (w8, 3, 5, 3)):
        c, cur, ref, at = w.ctx, w.cur, w.ref, w.at
        what = (R, coarse, w.ctx.bit_depth)
        if not coarse:
            assert w.counted(lambda: c.p_shape_frame(cur, ref, search_range=R, **at))[1] == (PAIR, F(NODES), search + 2 + 1), what
        kw = dict(search_range=R, coarse_range=coarse, **at)
        assert w.counted(lambda: c.p_tree_frame(cur, ref, **kw))[1] == (PAIR, 2 * MAPS, search + 2 + 2), what
        assert w.counted(lambda: c.p_tree_frame(cur, ref, with_shapes=True, **kw))[1] == (PAIR, 2 * MAPS + F(NODES), search + 2 + 2), what
        for shapes, merge in itertools.product((False, True), repeat=2):
            d = w.counted(lambda: c.p_tree_merge_frame(cur, ref, with_shapes=shapes, with_merge=merge, **kw))[1]
            assert d == (PAIR, 2 * MAPS + (shapes + merge) * F(NODES), search + 2 + 3), (what, shapes, merge)


# ---- 2. rejected calls move nothing ----------------------------------------------------------------------------------------------------------------------------

# every host form takes (ctx, cur, ref, stride, qp, range) and then pointers: an "in" (with the number of entries per CTU), an "out", or "centres"; the
# in / out slots are the families: an entry point with a pair per family rejects half a pair, and every entry point rejects a call without any family
HOST_FORMS = [
    ("fhevc_motion_search", 64, [("out", NODES)]),
    ("fhevc_motion_search_pu", 8, [("out", NODES), ("out", PUS)]),
    ("fhevc_motion_search_pu_small", 8, [("out", SMALL)]),
    ("fhevc_motion_search_pu_wide", 64, [("out", NODES), ("out", PUS), ("out", SMALL)]),
    ("fhevc_motion_centres", 14, [("out", 1)]),
    ("fhevc_motion_search_pu_centred", 8, [("centres", 1), ("out", NODES), ("out", PUS), ("out", SMALL)]),
    ("fhevc_motion_refine", 64, [("in", NODES), ("out", NODES)]),
    ("fhevc_motion_merge", 64, [("in", NODES), ("out", NODES)]),
    ("fhevc_motion_refine_pu", 8, [("in", PUS), ("out", PUS), ("in", SMALL), ("out", SMALL)]),
    ("fhevc_motion_refine_pu_wide", 64, [("in", NODES), ("out", NODES), ("in", PUS), ("out", PUS), ("in", SMALL), ("out", SMALL)]),
    ("fhevc_motion_refine_pu_centred", 8, [("centres", 1), ("in", NODES), ("out", NODES), ("in", PUS), ("out", PUS), ("in", SMALL), ("out", SMALL)]),
]


@pytest.mark.parametrize("name,limit,slots", HOST_FORMS, ids=[f[0] for f in HOST_FORMS])
def test_rejected_calls_move_nothing(w8, name, limit, slots):
    c, lib = w8.ctx, w8.ctx.lib
    fn = getattr(lib, name)
    cur, ref = w8.cur.ctypes.data + 2 * ORG, w8.ref.ctypes.data + 2 * ORG
    found = w8.found(4)
    vectors = {NODES: found[0], PUS: found[1], SMALL: found[2], 1: np.zeros(N, capi.MOTION_DTYPE)}
    bufs = [np.ascontiguousarray(vectors[k]) if kind != "out" else np.full(N * k * 16, CANARY, np.uint8) for kind, k in slots]
    ptrs = [b.ctypes.data for b in bufs]
    family = [i for i, (kind, _) in enumerate(slots) if kind != "centres"]
    good = dict(cur=cur, ref=ref, stride=STRIDE, qp=QP, R=min(4, limit))
    bad = [dict(qp=52), dict(R=0), dict(R=limit + 1), dict(stride=W - 1), dict(cur=None), dict(ref=None), dict(drop=family)]
    if any(kind == "in" for kind, _ in slots):
        bad += [dict(drop=[i]) for i in family]            # half an in / out pair
    for change in bad:
        a = dict(good, **{k: v for k, v in change.items() if k != "drop"})
        p = [None if i in change.get("drop", ()) else q for i, q in enumerate(ptrs)]
        before = c.stats()
        rc = fn(c.h, a["cur"], a["ref"], a["stride"], a["qp"], a["R"], *p)
        assert rc == capi.E_INVALID, change
        assert lib.fhevc_last_error(c.h).decode() != "", change
        assert all((b == CANARY).all() for b, (kind, _) in zip(bufs, slots) if kind == "out"), change
        after = c.stats()
        assert all(after[k] == before[k] for k in COUNTERS), (change, before, after)
    # the same call with nothing wrong is accepted and fills every output
    assert fn(c.h, cur, ref, STRIDE, QP, good["R"], *ptrs) == capi.OK
    assert all(not (b == CANARY).all() for b, (kind, _) in zip(bufs, slots) if kind == "out")


# ---- 3. the rejection that comes after the pair was staged ----------------------------------------------------------------------------------------------------

def test_a_late_rejection_leaves_the_context_usable(w8):
    """the SATD distortion covers ranges up to 8: fhevc_motion_search at 9 stages the pair and is then rejected by its device form"""
    c, lib = w8.ctx, w8.ctx.lib
    out = np.full(F(NODES), CANARY, np.uint8)
    launched = c.stats()["kernels_launched"]
    rc = lib.fhevc_motion_search(c.h, w8.cur.ctypes.data + 2 * ORG, w8.ref.ctypes.data + 2 * ORG, STRIDE, QP, 9, out.ctypes.data)
    assert rc == capi.E_INVALID and "SAD" in lib.fhevc_last_error(c.h).decode()
    assert (out == CANARY).all() and c.stats()["kernels_launched"] == launched
    again = c.motion_search(w8.cur, w8.ref, search_range=4, **w8.at)
    fresh = World(8)
    assert again.tobytes() == fresh.ctx.motion_search(fresh.cur, fresh.ref, search_range=4, **fresh.at).tobytes()
    assert (again["satd_best"] > 0).any()
    fresh.close()
