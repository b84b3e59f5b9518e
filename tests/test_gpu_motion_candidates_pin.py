"""Config 4 (P slices): the three neighbour stages on the MI355X -- k_motion_amvp.hip, k_motion_merge.hip, k_motion_merge_pu.hip -- against the REFERENCE's
own candidate lists, read from tests/golden/ref_motion_candidates.npz (what TComDataCU::fillMvpCand and TComDataCU::getInterMergeCandidates returned on
hand-set motion fields, and the reference's getCost table; tests/quality/gen_motion_candidates_golden.py).  The expected values are computed from the file
alone (motion_candidates_cases.amvp_expected / check_merge): no Python restatement of a list rule or of the geometry stands between the kernels and the
reference here.  tests/test_motion_candidates_pin.py holds the restatements and the host twin to the same file without a GPU."""
import numpy as np
import pytest

import motion_amvp_ref as ar
import motion_candidates_cases as cc
from fasthevc_amd import capi
from motion_gpu_helpers import CANARY, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

QDT, VDT, MDT = ar.QDT, ar.VDT, capi.MOTION_MERGE_DTYPE


class Guarded:
    """nbytes of device output between two canary-filled guards of 4 KiB, everything pre-filled with the canary"""
    GUARD = 4096

    def __init__(self, torch, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * self.GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + self.GUARD

    def result(self, dtype, shape):
        h = self.t.cpu().numpy()
        assert (h[:self.GUARD] == CANARY).all() and (h[self.GUARD + self.n:] == CANARY).all(), "a guard around the output was written"
        return h[self.GUARD:self.GUARD + self.n].copy().view(dtype).reshape(shape)


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    c = capi.Context(cc.W, cc.H, 8, max_frames=2)
    yield c
    c.close()


def test_amvp_kernel_prices_on_the_references_candidates(torch_cuda, ctx):
    """every draw of the file as one batch of picture pairs, all three families, both outputs, at three QPs: px, py, idx and bits of the predictor record
    are the first index of least bits over the reference's two candidates, cost_best is min(satd_best + the reference's getCost[bits], 0xFFFFFFFE)"""
    torch = torch_cuda
    data = cc.load()
    D = len(cc.KINDS)
    rng = np.random.default_rng(99)
    rec = {f: cc.records(rng, data[f"mv_{f}"], data[f"marker_{f}"]) for f in cc.FAMILIES}
    held = {f: to_dev(torch, a) for f, a in rec.items()}
    for qp in (0, ar.DRAW_QP, 51):
        outs = {f: Guarded(torch, D * cc.N * cc.PER[f] * 16) for f in cc.FAMILIES}
        mvps = {f: Guarded(torch, D * cc.N * cc.PER[f] * 8) for f in cc.FAMILIES}
        torch.cuda.synchronize()
        ctx.motion_amvp_device(D + 1, *[held[f].data_ptr() for f in cc.FAMILIES], *[outs[f].ptr for f in cc.FAMILIES], *[mvps[f].ptr for f in cc.FAMILIES], qp=qp)
        torch.cuda.synchronize()
        high = set()
        for f in cc.FAMILIES:
            shape = (D, cc.N, cc.PER[f])
            got, mvp = outs[f].result(QDT, shape), mvps[f].result(VDT, shape)
            won, bits = cc.check_amvp(f, rec[f], data[f"ref_{f}"], data["cost"][qp], got, mvp, qp)
            assert won >= 8, (f, won)                                                      # both list slots are seen through the kernel
            assert int(cc.compared(f, data[f"marker_{f}"]).sum()) == cc.COMPARED[f]
            for name in ("satd_int", "satd_best", "mvx", "mvy"):                           # everything but the price is copied
                assert np.array_equal(got[name][got["cost_best"] != ar.MARK], rec[f][name][got["cost_best"] != ar.MARK]), (f, name)
            high |= set(bits[bits >= 39].tolist())
        assert len(high) >= 8 and max(high) == 66, sorted(high)                            # table entries above 38 against the reference's numbers


def test_merge_kernels_choose_from_the_references_lists(torch_cuda, ctx):
    """fhevc_motion_merge_device and fhevc_motion_merge_pu_device at max_range 8 on the merge draws, the stored node records as the refined input, on a fixed
    pair of random 8-bit planes: the record's vector is the reference's list entry at idx, num the length of the reference's list up to and including its
    first filled zero, src = 5 exactly where that entry is the fill"""
    torch = torch_cuda
    data = cc.load()
    planes = np.random.default_rng(168152).integers(0, 256, size=(2, cc.H, cc.W)).astype(np.uint8)
    d_luma = to_dev(torch, planes)
    rng = np.random.default_rng(7)
    seen = dict.fromkeys(cc.FAMILIES, 0)
    nums, fills = set(), 0
    for d in cc.MERGE_DRAWS:
        refined = cc.records(rng, data["mv_nodes"][d], data["marker_nodes"][d])
        d_ref = to_dev(torch, refined)
        outs = {f: Guarded(torch, cc.N * cc.PER[f] * 16) for f in cc.FAMILIES}
        torch.cuda.synchronize()
        ctx.motion_merge_device(d_luma.data_ptr(), 1, cc.W, cc.W * cc.H, 2, d_ref.data_ptr(), outs["nodes"].ptr, qp=4, max_range=cc.MERGE_RANGE)
        ctx.motion_merge_pu_device(d_luma.data_ptr(), 1, cc.W, cc.W * cc.H, 2, d_ref.data_ptr(), outs["pu"].ptr, outs["small"].ptr, qp=4, max_range=cc.MERGE_RANGE)
        torch.cuda.synchronize()
        for f in cc.FAMILIES:
            got = outs[f].result(MDT, (cc.N, cc.PER[f]))
            seen[f] += cc.check_merge(f, data[f"ref_{f}"][d], got, d)
            ok = got["num"] > 0
            nums |= set(got["num"][ok].tolist())
            fills += int((got["src"][ok] == 5).sum())
    assert seen == {f: n for f, n in cc.COMPARED_MERGE.items()}, seen
    # bits are cheap at qp 4: winners behind index 0 and filled zeros both occur, in lists of every length
    assert nums == {1, 2, 3, 4, 5} and fills > 0
