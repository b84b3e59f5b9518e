"""Config 4 (P slices): every search range 1..64 through the integer motion searches and the quarter-sample refinements on the MI355X.  How the
kernels lay out their work depends on the range's residues -- where the 8-sample chunks fall in the LDS window (delta = (8 - R mod 8) mod 8, dword
stores when delta is 0 or 4, bytes otherwise), how many vectors the last dx group masks ((2R+1) mod 4), how far the last dy block is moved up
((2R+1) mod DB, DB = 6, 2 or 4 by the families asked for), how many lanes of the last round repeat the last item -- so every range runs, on a
104 x 88 picture (one whole CTU, one 40 wide, one 24 tall, the corner) whose windows reach a replicated border at every range, three pictures per
clip.  Expected records come from tests/motion_range_sweep.py (one +-64 SAD volume per CTU gives every range; pinned by
tests/test_motion_range_sweep_ref.py, which also asserts that winners sit on all four edges of the window at every range).  Every valid entry of
every CTU is compared in all five fields, markers included; the number compared is asserted against the geometry's count; outputs lie between
canaries.  Cases are blocks of 8 consecutive ranges."""
import numpy as np
import pytest

import motion_range_sweep as sw
from fasthevc_amd import capi
from motion_gpu_helpers import Guarded, pel_batch, same, to_dev, torch_cuda  # noqa: F401
from test_gpu_motion_pu_wide import run_dev, square_search
from test_gpu_motion_refine_pu_wide import refine_dev

pytestmark = pytest.mark.gpu

FAMS, PER = sw.FAMS, sw.PER
NF = sw.NF
WIDE_BLOCKS = [tuple(range(lo, lo + 8)) for lo in range(9, 65, 8)]          # 9..16, .., 57..64
ALL_BLOCKS = [tuple(range(lo, lo + 8)) for lo in range(1, 65, 8)]           # 1..8, .., 57..64
DELTA4_BLOCK = (12, 20, 28, 36, 44, 52, 60, 64)
block_id = lambda b: f"R{b[0]}-{b[-1]}"
# the instantiations of the byte kernel besides all three outputs (FAM 7, DB 2): each family alone (DB 6 / 2 / 4), nodes plus small PUs (FAM 5, DB 4)
SUBSETS = (("nodes",), ("pu",), ("small",), ("nodes", "small"))


class Clip:
    """a sweep clip on the device: int16 planes in TComPicYuv's layout, or tight uint8 planes (8 bit only)"""

    def __init__(self, torch, name, bd, u8=False):
        self.name, self.bd, self.qp = name, bd, sw.clip_qp(name, bd)
        if u8:
            assert bd == 8
            flat, self.org, self.stride, self.fs, self.sb = np.stack(sw.clip(name)), 0, sw.W, sw.W * sw.H, 1
        else:
            flat, self.org, self.stride, self.fs = pel_batch(sw.planes(name, bd))
            self.sb = 2
        self.flat = flat
        self.d_luma = to_dev(torch, flat)
        self.ptr = self.d_luma.data_ptr() + self.sb * self.org

    def search(self, torch, ctx, R, fams=FAMS):
        return run_dev(torch, ctx, self.flat, self.org, self.stride, self.fs, NF, self.sb, self.qp, R, fams=fams, d_luma=self.d_luma)

    def square(self, torch, ctx, R):
        return square_search(torch, ctx, self.ptr, self.sb, self.stride, self.fs, NF, self.qp, R, ctx.num_ctus)


def held(got, exp, what):
    """every field of every entry of the families in got, markers included, and the bytes; -> {family: valid entries compared}"""
    n = {}
    for f in got:
        same(got[f], exp[f], (what, f))
        assert got[f].tobytes() == exp[f].tobytes(), (what, f)
        n[f] = int((got[f]["cost_best"] != sw.MARKER).sum())
    return n


def counts(fams=FAMS):
    """valid entries of a device call over the clip's two pairs, from the geometry"""
    c = sw.valid_counts()
    return {f: (NF - 1) * c[f] for f in fams}


# ---- (a) the byte path: 8-bit context, int16 and uint8 planes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u8", [False, True], ids=["int16", "uint8"])
@pytest.mark.parametrize("block", WIDE_BLOCKS, ids=block_id)
def test_byte_path_every_instantiation(oracle, torch_cuda, block, u8):
    torch = torch_cuda
    ctx = capi.Context(sw.W, sw.H, 8, max_frames=NF)
    for name in sw.CLIPS:
        clip = Clip(torch, name, 8, u8)
        for R in block:
            exp = sw.expected(oracle, name, 8, R)
            got = clip.search(torch, ctx, R)
            assert held(got, exp, (name, R, "all three")) == counts(), (name, R)
            for fams in SUBSETS:
                sub = clip.search(torch, ctx, R, fams=fams)
                assert held(sub, exp, (name, R, fams)) == counts(fams), (name, R, fams)
                for f in fams:
                    assert sub[f].tobytes() == got[f].tobytes(), (name, R, fams, f)
    ctx.close()


# ---- (b) the stateful square entry point ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", WIDE_BLOCKS, ids=block_id)
def test_square_entry_with_the_range_changing_from_call_to_call(oracle, torch_cuda, block):
    """fhevc_motion_search_device in SAD mode (k_motion_wide.hip) rebuilds its cost table on every call: the range and the QP change with each call,
    upwards through the block on one clip, downwards on the next"""
    torch = torch_cuda
    ctx = capi.Context(sw.W, sw.H, 8, max_frames=NF)
    clips = [Clip(torch, name, 8) for name in sw.CLIPS]
    order = [(c, R) for R in block for c in clips[:2]] + [(clips[2], R) for R in reversed(block)] + [(clips[0], block[0])]
    for clip, R in order:
        exp = sw.expected(oracle, clip.name, 8, R)
        got = clip.square(torch, ctx, R)
        assert held({"nodes": got}, exp, (clip.name, R, "square")) == counts(("nodes",)), (clip.name, R)
        assert got.tobytes() == clip.search(torch, ctx, R)["nodes"].tobytes(), (clip.name, R)
    ctx.close()


# ---- (c) the generic MR = 64 layouts ------------------------------------------------------------------------------------------------------------------------

def generic_block(oracle, torch, bd, block):
    ctx = capi.Context(sw.W, sw.H, bd, max_frames=NF)
    for name in sw.CLIPS:
        clip = Clip(torch, name, bd)
        for R in block:
            exp = sw.expected(oracle, name, bd, R)
            got = clip.search(torch, ctx, R)
            assert held(got, exp, (name, bd, R)) == counts(), (name, bd, R)
            sq = clip.square(torch, ctx, R)
            assert held({"nodes": sq}, exp, (name, bd, R, "square")) == counts(("nodes",)), (name, bd, R)
    ctx.close()


@pytest.mark.parametrize("block", WIDE_BLOCKS, ids=block_id)
def test_generic_path_10_bit(oracle, torch_cuda, block):
    generic_block(oracle, torch_cuda, 10, block)


def test_generic_path_12_bit_where_the_window_starts_a_dword_early(oracle, torch_cuda):
    generic_block(oracle, torch_cuda, 12, DELTA4_BLOCK)


@pytest.mark.parametrize("block", WIDE_BLOCKS, ids=block_id)
def test_generic_path_on_8_bit_planes_equals_the_byte_path(oracle, torch_cuda, monkeypatch, block):
    """FHEVC_PU_WIDE=generic is read when a context is created"""
    torch = torch_cuda
    ctx = capi.Context(sw.W, sw.H, 8, max_frames=NF)
    monkeypatch.setenv("FHEVC_PU_WIDE", "generic")
    ctx_generic = capi.Context(sw.W, sw.H, 8, max_frames=NF)
    monkeypatch.delenv("FHEVC_PU_WIDE")
    for name in sw.CLIPS:
        clip = Clip(torch, name, 8)
        for R in block:
            exp = sw.expected(oracle, name, 8, R)
            there = clip.search(torch, ctx_generic, R)
            assert held(there, exp, (name, R, "generic")) == counts(), (name, R)
            here = clip.search(torch, ctx, R)
            for f in FAMS:
                assert there[f].tobytes() == here[f].tobytes(), (name, R, f)
    ctx.close()
    ctx_generic.close()


# ---- (d) the MR = 8 kernels ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["sad", "satd"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_small_ranges_through_the_three_entry_points(oracle, torch_cuda, bd, mode):
    torch = torch_cuda
    ctx = capi.Context(sw.W, sw.H, bd, max_frames=NF)
    ctx.set_motion_distortion(mode)
    n = ctx.num_ctus
    for name in sw.CLIPS:
        clip = Clip(torch, name, bd)
        for R in range(1, 9):
            exp = sw.expected(oracle, name, bd, R, sad=mode == "sad")
            g = {f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}
            alone = Guarded(torch, (NF - 1) * n * 85 * 16)
            torch.cuda.synchronize()
            ctx.motion_search_device(clip.ptr, 2, clip.stride, clip.fs, NF, alone.ptr, qp=clip.qp, search_range=R)
            ctx.motion_search_pu_device(clip.ptr, 2, clip.stride, clip.fs, NF, g["pu"].ptr, g["nodes"].ptr, qp=clip.qp, search_range=R)
            ctx.motion_search_pu_small_device(clip.ptr, 2, clip.stride, clip.fs, NF, g["small"].ptr, qp=clip.qp, search_range=R)
            torch.cuda.synchronize()
            got = {f: g[f].result((NF - 1, n, PER[f])) for f in FAMS}
            assert held(got, exp, (name, bd, mode, R)) == counts(), (name, bd, mode, R)
            assert held({"nodes": alone.result((NF - 1, n, 85))}, exp, (name, bd, mode, R, "square")) == counts(("nodes",))
            if mode == "sad":
                wide = clip.search(torch, ctx, R)
                for f in FAMS:
                    assert wide[f].tobytes() == got[f].tobytes(), (name, bd, R, f)
    ctx.close()


# ---- (e) the refinements --------------------------------------------------------------------------------------------------------------------------------------

REFINE_CLIP = "slow"


@pytest.mark.parametrize("block", ALL_BLOCKS, ids=block_id)
@pytest.mark.parametrize("bd", [8, 10])
def test_refinement_behind_the_search_at_every_max_range(oracle, torch_cuda, monkeypatch, bd, block):
    """fhevc_motion_refine_pu_wide_device behind fhevc_motion_search_pu_wide_device on one non-default stream, all three families, at max_range = R
    around the search's vectors at R, and around those of range min(64, R + 3): what exceeds max_range comes out as markers, the rest as the
    restatement refines it.  From R = 9 on a context that stages the whole window (FHEVC_REFINE_PU_STAGE=full, read when a context is created)
    writes the same bytes as the default one, which stages the part max_range reaches"""
    torch = torch_cuda
    ctx = capi.Context(sw.W, sw.H, bd, max_frames=NF)
    monkeypatch.setenv("FHEVC_REFINE_PU_STAGE", "full")
    ctx_full = capi.Context(sw.W, sw.H, bd, max_frames=NF)
    monkeypatch.delenv("FHEVC_REFINE_PU_STAGE")
    clip = Clip(torch, REFINE_CLIP, bd)
    memo = sw.refine_memo(oracle, REFINE_CLIP, bd)
    n = ctx.num_ctus
    st = torch.cuda.Stream()
    for R in block:
        for R_in in (R, min(64, R + 3)):
            mid = {f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}
            out = {f: Guarded(torch, (NF - 1) * n * PER[f] * 16) for f in FAMS}
            torch.cuda.synchronize()
            ctx.motion_search_pu_wide_device(clip.ptr, 2, clip.stride, clip.fs, NF, mid["nodes"].ptr, mid["pu"].ptr, mid["small"].ptr, stream=st.cuda_stream,
                                             qp=clip.qp, search_range=R_in)
            ctx.motion_refine_pu_wide_device(clip.ptr, 2, clip.stride, clip.fs, NF, mid["nodes"].ptr, out["nodes"].ptr, mid["pu"].ptr, out["pu"].ptr,
                                             mid["small"].ptr, out["small"].ptr, stream=st.cuda_stream, qp=clip.qp, max_range=R)
            torch.cuda.synchronize()
            vec = {f: mid[f].result((NF - 1, n, PER[f])) for f in FAMS}
            held(vec, sw.expected(oracle, REFINE_CLIP, bd, R_in), (bd, R_in, "search"))
            got = {f: out[f].result((NF - 1, n, PER[f])).view(sw.QDT) for f in FAMS}
            exp = memo.expected(vec, R)
            kinds = np.zeros(2, np.int64)
            for f in FAMS:
                for k in sw.QDT.names:
                    bad = got[f][k] != exp[f][k]
                    assert not bad.any(), (bd, R, R_in, f, k, np.argwhere(bad)[:5].tolist(), got[f][k][bad][:5].tolist(), exp[f][k][bad][:5].tolist())
                searched = vec[f]["cost_best"] != sw.MARKER
                too_long = searched & ((np.abs(vec[f]["mvx"].astype(np.int64)) > R) | (np.abs(vec[f]["mvy"].astype(np.int64)) > R))
                mark = got[f]["cost_best"] == sw.MARKER
                assert np.array_equal(mark, too_long | ~searched), (bd, R, R_in, f)
                assert (got[f]["satd_int"][mark] == sw.MARKER).all() and (got[f]["mvx"][mark] == 0).all() and (got[f]["mvy"][mark] == 0).all()
                if R_in == R:
                    assert not too_long.any() and int((~mark).sum()) == counts()[f], (bd, R, f)
                kinds += [int(too_long.sum()), int((searched & ~too_long).sum())]
            if R_in > R:
                assert kinds.min() > 0, (bd, R, R_in, kinds.tolist())          # both kinds occurred: refused for its length, and refined
            if R >= 9:
                there = refine_dev(torch, ctx_full, clip.ptr, 2, clip.stride, clip.fs, NF, clip.qp, R, vec)
                for f in FAMS:
                    assert there[f].tobytes() == got[f].tobytes(), (bd, R, R_in, f)
    ctx.close()
    ctx_full.close()
