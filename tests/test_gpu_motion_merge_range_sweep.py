"""Config 4 (P slices): every max_range 1..64 through the three kernels that stage only the part of their LDS window that max_range reaches
(refine_stage_window_reach of k_refine_tile.h: k_motion_merge.hip, k_motion_merge_pu.hip, k_motion_skip.hip) on the MI355X.  What is staged depends on
skip = MR - max_range and on skip mod 4, in the static MR = 8 layout (max_range <= 8) and in the dynamic MR = 64 layout; every cell outside it is stale.

The inputs are tests/motion_merge_sweep_cases.py's (tests/test_motion_merge_range_sweep_ref.py asserts without a GPU what they probe), on a 168 x 152
picture: corner pairs -- the current picture is the reference's prediction at the corner (+-(4R + 3), +-(4R + 3)) of the reach, whose filters read the
outermost staged row and column for their value; every entry with a neighbour must come out at distortion 0 -- and a draw of refined records on
noise.  Every record is compared byte for byte with the CPU restatements (motion_merge_ref, motion_merge_pu_ref, motion_skip_ref), the corner pairs
also with the closed form, and the number of entries compared is asserted against the geometry's counts.  Outputs lie between canaries.  No two
launches show the same reference samples: a persistent workgroup that staged them at a larger range would have left them behind in the unstaged cells.

Instantiations, each at every R: uint8 planes at 8 bit, int16 planes at 10 bit (the packed form), int16 planes at 12 bit (the 32-bit form of the two
merge kernels; the skip kernel has no packed parameter and runs every R at 12 bit all the same)."""
import numpy as np
import pytest

import motion_merge_ref as mg
import motion_merge_sweep_cases as cs
import motion_skip_ref as sk
from fasthevc_amd import capi, frames
from motion_gpu_helpers import Guarded, pel, pel_batch, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

MDT, KDT = cs.MDT, cs.KDT
INSTANCES = [(np.uint8, 8), (np.int16, 10), (np.int16, 12)]
instance_id = lambda i: f"{np.dtype(i[0]).name}-{i[1]}bit"
BLOCKS4 = [tuple(range(lo, lo + 4)) for lo in range(1, 65, 4)]
BLOCKS8 = [tuple(range(lo, lo + 8)) for lo in range(1, 65, 8)]
EDGE_BLOCKS = [BLOCKS8[0], BLOCKS8[-1]]                     # 1..8: the MR = 8 layout; 57..64: the MR = 64 layout
block_id = lambda b: f"R{b[0]}-{b[-1]}"
PER = {"nodes": 85, "pu": 124, "small": 384, "skip": 85}
VALID = {"nodes": 513, "pu": 648, "small": 2316}            # valid entries of the picture: the sums of test_motion_merge_range_sweep_ref.COUNTS
FED = {"nodes": 509, "pu": 576, "small": 2232, "skip": 509}   # ... and those with an available neighbour


class Pair:
    """(reference, current) as a batch of two frames on the device: tight uint8 planes or int16 planes in TComPicYuv's layout; guarded: poisoned margins,
    odd origin and odd stride (frames.guarded_plane), so that no chunk takes the one-load path"""

    def __init__(self, torch, ref, cur, dtype, bd, guarded=False):
        self.sb = np.dtype(dtype).itemsize
        if guarded:
            flat, self.org, self.stride, self.fs = frames.guarded_plane([ref, cur], bit_depth=bd, dtype=dtype, extra_stride=3, shift=1, frame_gap=5, poison=77)
            assert self.stride % 2 == 1 and self.org % 2 == 1
        elif self.sb == 1:
            flat, self.org, self.stride, self.fs = np.stack([ref, cur]).astype(np.uint8), 0, cs.W, cs.W * cs.H
        else:
            flat, self.org, self.stride, self.fs = pel_batch([ref, cur])
        self.d = to_dev(torch, flat)
        self.ptr = self.d.data_ptr() + self.sb * self.org


class Launch:
    """the three stages of one pair at one max_range: buffers first, go() queues the launches without synchronising, results() reads them back.
    families: which of the PU families fhevc_motion_merge_pu_device writes; merge_in: the skip stage's input records (the expected merge records)"""

    def __init__(self, torch, pair, refined, merge_in, merge_qp, skip_qp, R, families=("pu", "small"), merge2=None):
        self.pair, self.R, self.qps, self.families = pair, R, (merge_qp, skip_qp), families
        self.d_refined, self.d_merge = to_dev(torch, refined), to_dev(torch, merge_in)
        self.d_merge2 = to_dev(torch, merge2) if merge2 is not None else None
        self.out = {f: Guarded(torch, cs.N * PER[f] * 16) for f in ("nodes", "skip") + tuple(families)}
        if merge2 is not None:
            self.out["skip2"] = Guarded(torch, cs.N * 85 * 16)

    def go(self, ctx, stream=None):
        p, (mq, sq), o = self.pair, self.qps, self.out
        a = (p.ptr, p.sb, p.stride, p.fs, 2)
        ctx.motion_merge_device(*a, self.d_refined.data_ptr(), o["nodes"].ptr, stream=stream, qp=mq, max_range=self.R)
        ctx.motion_merge_pu_device(*a, self.d_refined.data_ptr(), o["pu"].ptr if "pu" in o else None, o["small"].ptr if "small" in o else None, stream=stream,
                                   qp=mq, max_range=self.R)
        ctx.motion_skip_device(*a, self.d_merge.data_ptr(), o["skip"].ptr, stream=stream, qp=sq, max_range=self.R)
        if self.d_merge2 is not None:
            ctx.motion_skip_device(*a, self.d_merge2.data_ptr(), o["skip2"].ptr, stream=stream, qp=sq, max_range=self.R)
        return self

    def results(self):
        return {f: g.result((cs.N, PER[f.rstrip("2")])).view(KDT if f.startswith("skip") else MDT) for f, g in self.out.items()}


def held(got, exp, what):
    """every byte of every record of the families in got -> {family: valid entries compared}"""
    n = {}
    for f, g in got.items():
        (sk if f.startswith("skip") else mg).same(g, exp[f], (what, f))
        assert g.tobytes() == exp[f].tobytes(), (what, f)
        n[f] = int((g["coef_max"] != sk.MARK).sum()) if f.startswith("skip") else int((g["num"] > 0).sum())
    return n


def corner_launches(torch, case, dtype, bd, R, corners, guarded=False):
    out = {}
    for corner in corners:
        c = case["corners"][corner]
        pair = Pair(torch, case["ref"], c["cur"], dtype, bd, guarded)
        out[corner] = Launch(torch, pair, c["refined"], c["exp"]["nodes"], case["qp"], cs.SKIP_QP, R)
    return out


def check_corner_results(launches, case, what):
    """byte for byte against the restatements, against the closed form, and the counts"""
    for corner, launch in launches.items():
        c, got = case["corners"][corner], launch.results()
        n = held(got, c["exp"], (what, corner))
        assert {f: n[f] for f in VALID} == VALID and n["skip"] == VALID["nodes"], (what, corner, n)
        assert cs.check_corner(got, c["q"], case["c1"]) == FED, (what, corner)


# ---- (a) the corner pairs: every R, every corner, every instantiation -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", BLOCKS4, ids=block_id)
@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_corner_pairs_at_every_max_range(oracle, torch_cuda, inst, block):
    """per R the four corners, all three kernels each; at the block's first R each PU family also alone (another instantiation of the PU kernel's
    passes), which must write the bytes it writes beside the other"""
    torch, (dtype, bd) = torch_cuda, inst
    ctx = capi.Context(cs.W, cs.H, bd, max_frames=2)
    for R in block:
        case = cs.corner_case(oracle, bd, R)
        launches = corner_launches(torch, case, dtype, bd, R, cs.CORNERS)
        alone = {}
        if R == block[0]:
            for fam, corner in (("pu", cs.CORNERS[0]), ("small", cs.CORNERS[3])):
                c = case["corners"][corner]
                alone[fam] = (corner, Launch(torch, launches[corner].pair, c["refined"], c["exp"]["nodes"], case["qp"], cs.SKIP_QP, R, families=(fam,)))
        torch.cuda.synchronize()
        for launch in launches.values():
            launch.go(ctx)
        for _, launch in alone.values():
            launch.go(ctx)
        torch.cuda.synchronize()
        check_corner_results(launches, case, (inst, R))
        for fam, (corner, launch) in alone.items():
            got = launch.results()
            assert set(got) == {"nodes", "skip", fam} and got[fam].tobytes() == case["corners"][corner]["exp"][fam].tobytes(), (inst, R, fam)
    ctx.close()


# ---- (b) the draw: every R, every instantiation -----------------------------------------------------------------------------------------------------------------

def check_draw_results(launch, case, R, what):
    got = launch.results()
    exp = dict(case["exp"], skip2=case["skip2"])
    n = held(got, exp, what)
    assert {f: n[f] for f in VALID} == VALID, (what, n)
    reach = 4 * R + 3
    # the skip stage ran at the winners' vectors -- the limit of the reach among them -- and on records in its own scheme: on the limit in every sign,
    # one quarter sample beyond it, markers
    won = case["exp"]["nodes"]
    assert n["skip"] == int(((won["num"] > 0) & (won["cost_best"] != mg.MARK)).sum()) > 0, what
    m, s2 = case["merge2"], got["skip2"]
    ok = s2["coef_max"] != sk.MARK
    assert all((ok & hit).any() for hit in (s2["mvx"] == reach, s2["mvx"] == -reach, s2["mvy"] == reach, s2["mvy"] == -reach)), what
    beyond = (np.abs(m["mvx"].astype(np.int64)) == reach + 1) | (np.abs(m["mvy"].astype(np.int64)) == reach + 1)
    assert (~ok & beyond).any() and (~ok & (m["cost_best"] == mg.MARK)).any() and not (ok & beyond).any(), what
    for fam in ("nodes", "pu", "small"):
        g = got[fam]
        live = g["num"] > 0
        assert set(np.unique(g["num"][live])) == {1, 2, 3, 4, 5}, (what, fam)
        assert (live & (np.abs(g["mvx"]) == reach)).any() and (live & (np.abs(g["mvy"]) == reach)).any(), (what, fam)


@pytest.mark.parametrize("block", BLOCKS8, ids=block_id)
@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_the_draw_at_every_max_range(oracle, torch_cuda, inst, block):
    torch, (dtype, bd) = torch_cuda, inst
    ctx = capi.Context(cs.W, cs.H, bd, max_frames=2)
    for R in block:
        case = cs.draw_case(oracle, bd, R)
        launch = Launch(torch, Pair(torch, *case["pics"], dtype, bd), case["refined"], case["exp"]["nodes"], cs.DRAW_QP, cs.SKIP_QP, R, merge2=case["merge2"])
        torch.cuda.synchronize()
        launch.go(ctx)
        torch.cuda.synchronize()
        check_draw_results(launch, case, R, (inst, R))
    ctx.close()


# ---- (c) max_range changing from call to call on one context and one stream -------------------------------------------------------------------------------------

CHANGING = (8, 9, 8, 9, 7, 10, 1, 64, 5, 33, 2, 12, 8)


@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_max_range_changing_from_call_to_call_without_synchronisation(oracle, torch_cuda, inst):
    """8 -> 9 and 9 -> 8 and wider jumps: static against dynamic LDS and another grid size with each call, every launch queued on one non-default stream
    before the first result is read; every step has a picture of its own and alternates between the two corners that touch all four sides"""
    torch, (dtype, bd) = torch_cuda, inst
    ctx = capi.Context(cs.W, cs.H, bd, max_frames=2)
    steps = []
    for i, R in enumerate(CHANGING):
        corner = cs.CORNERS[0] if i % 2 == 0 else cs.CORNERS[3]
        case = cs.corner_case(oracle, bd, R, variant="changing", extra=i, corners=(corner,))
        steps.append((R, case, corner_launches(torch, case, dtype, bd, R, (corner,))))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for R, case, launches in steps:
        for launch in launches.values():
            launch.go(ctx, stream=st.cuda_stream)
    torch.cuda.synchronize()
    for i, (R, case, launches) in enumerate(steps):
        check_corner_results(launches, case, (inst, "step", i, R))
    ctx.close()


# ---- (d) the per-sample staging path: poisoned margins, odd origin, odd stride ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["corner", "draw"])
@pytest.mark.parametrize("block", EDGE_BLOCKS, ids=block_id)
@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_guarded_planes_at_the_ranges_of_both_layouts(oracle, torch_cuda, inst, block, kind):
    """no row of such a plane is aligned, so every chunk is staged sample by sample; what lies outside the picture is poison.  The corner pairs run the
    two corners that between them touch all four sides of the staged part"""
    torch, (dtype, bd) = torch_cuda, inst
    ctx = capi.Context(cs.W, cs.H, bd, max_frames=2)
    for R in block:
        if kind == "corner":
            case = cs.corner_case(oracle, bd, R, variant="guarded", corners=(cs.CORNERS[0], cs.CORNERS[3]))
            launches = corner_launches(torch, case, dtype, bd, R, case["corners"], guarded=True)
        else:
            case = cs.draw_case(oracle, bd, R, variant="guarded")
            pair = Pair(torch, *case["pics"], dtype, bd, guarded=True)
            launches = {None: Launch(torch, pair, case["refined"], case["exp"]["nodes"], cs.DRAW_QP, cs.SKIP_QP, R, merge2=case["merge2"])}
        torch.cuda.synchronize()
        for launch in launches.values():
            launch.go(ctx)
        torch.cuda.synchronize()
        if kind == "corner":
            check_corner_results(launches, case, (inst, R, "guarded"))
        else:
            check_draw_results(launches[None], case, R, (inst, R, "guarded"))
    ctx.close()


# ---- (e) the host forms at a partly staged window of each layout --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,bd,corner", [(3, 10, cs.CORNERS[1]), (21, 8, cs.CORNERS[2])])
def test_host_forms_equal_the_device_forms(oracle, torch_cuda, R, bd, corner):
    torch = torch_cuda
    case = cs.corner_case(oracle, bd, R, variant="host", corners=(corner,))
    c = case["corners"][corner]
    ctx = capi.Context(cs.W, cs.H, bd, max_frames=2)
    launches = corner_launches(torch, case, np.int16, bd, R, (corner,))
    torch.cuda.synchronize()
    launches[corner].go(ctx)
    torch.cuda.synchronize()
    check_corner_results(launches, case, ("device", R))
    dev = launches[corner].results()
    (rb, org, stride), (cb, _, _) = pel(case["ref"]), pel(c["cur"])
    nodes = ctx.motion_merge(cb, rb, c["refined"], org, stride, qp=case["qp"], max_range=R)
    pus, small = ctx.motion_merge_pu(cb, rb, c["refined"], org, stride, qp=case["qp"], max_range=R)
    skip = ctx.motion_skip(cb, rb, nodes, org, stride, qp=cs.SKIP_QP, max_range=R)
    host = {"nodes": nodes, "pu": pus, "small": small, "skip": skip}
    for f in host:
        assert host[f].tobytes() == dev[f].tobytes(), (R, f)
    assert cs.check_corner(host, c["q"], case["c1"]) == FED
    ctx.close()
