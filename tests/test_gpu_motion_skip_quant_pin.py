"""Config 4 (P slices): the zero-residual stage (k_motion_skip.hip) on the MI355X against the numbers the REFERENCE's own transform and quantiser gave for
the same nodes (tests/golden/ref_quant.npz, written by tests/quality/gen_quant_golden.py) -- directly, not through the Python restatement: coef_max,
level_sum, nonzero and bit 0 for equality; bit 1 as the sufficient condition it is (set -> the reference's RDOQ coded nothing in any TU of the node).
The clips are regenerated (motion_skip_quant_cases.pictures) and held to the SHA-256 in the file; the merge records are the stored ones.  Needs only the
fixture.  128 x 64: every level's transform mapping, two CTUs through the persistent loop."""
import numpy as np
import pytest

import motion_skip_quant_cases as qc
from fasthevc_amd import capi, frames
from motion_gpu_helpers import CANARY, pel, to_dev, torch_cuda  # noqa: F401  (torch_cuda: a fixture)

pytestmark = pytest.mark.gpu

MDT, KDT = capi.MOTION_MERGE_DTYPE, capi.MOTION_SKIP_DTYPE
INVALID = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF, 0, 0, 0, 0)        # include/fasthevc.h: the record of a node that is not valid
GUARD = 4096
_CACHE = {}


@pytest.fixture(scope="module")
def quant_golden():
    return np.load(qc.GOLDEN)


def clip(g, bd):
    if bd not in _CACHE:
        pics = qc.pictures(bd)
        assert qc.picture_hash(pics) == bytes(g[f"sha256_{bd}"]).hex()
        merges = np.ascontiguousarray(g[f"merge_{bd}"]).view(MDT).reshape(len(qc.RANGES), qc.CTUS, 85)
        _CACHE[bd] = (pics, merges)
    return _CACHE[bd]


def check(got, g, bd, r, qi, merge, what):
    """got [CTUS, 85] skip records against the recorded numbers of bit depth bd, range index r, QP index qi"""
    ok = qc.valid(merge, qc.RANGES[r])
    assert ok.sum() > 100 and (~ok).sum() > 20
    for ctu, k in np.argwhere(~ok):
        assert tuple(got[ctu, k]) == INVALID, (what, ctu, k, got[ctu, k])
    level_sum, nonzero = g[f"level_sum_{bd}"][r, :, :, qi], g[f"nonzero_{bd}"][r, :, :, qi]
    for field, rec in (("coef_max", g[f"coef_max_{bd}"][r]), ("level_sum", level_sum), ("nonzero", nonzero)):
        bad = ok & (got[field] != rec)
        assert not bad.any(), (what, field, np.argwhere(bad)[:5].tolist(), got[field][bad][:5].tolist(), rec[bad][:5].tolist())
    flags = got["flags"][ok]
    assert np.array_equal((flags & 1) != 0, level_sum[ok] == 0), what                                  # bit 0: xQuant codes no luma coefficient
    assert not (((flags & 2) != 0) & (g[f"rdoq_zero_{bd}"][r, :, :, qi][ok] == 0)).any(), what         # bit 1 -> RDOQ codes none either
    assert ((flags & 0xFC) == 0).all() and ((flags & 2) <= 2 * (flags & 1)).all() and (got["pad"] == 0).all(), what
    assert np.array_equal(got["mvx"][ok], merge["mvx"][ok]) and np.array_equal(got["mvy"][ok], merge["mvy"][ok]), what
    return flags


@pytest.mark.parametrize("qp", qc.NODE_QPS)
@pytest.mark.parametrize("max_range", qc.RANGES)
@pytest.mark.parametrize("dtype,bd", [(np.int16, 8), (np.uint8, 8), (np.int16, 10), (np.int16, 12)])
def test_the_kernel_gives_the_references_numbers(torch_cuda, quant_golden, dtype, bd, max_range, qp):
    torch = torch_cuda
    pics, merges = clip(quant_golden, bd)
    r, qi = qc.RANGES.index(max_range), qc.NODE_QPS.index(qp)
    sb = np.dtype(dtype).itemsize
    # margins, stride padding and the gap between the pictures hold poison: nothing outside a picture is read for its value
    flat, origin, stride, fstride = frames.guarded_plane(pics, bit_depth=bd, dtype=dtype, poison=bd + max_range)
    d_luma, d_merge = to_dev(torch, flat), to_dev(torch, merges[r])
    n = qc.CTUS * 85 * 16
    out = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")          # the records between two canary-filled guards
    ctx = capi.Context(qc.W, qc.H, bd, max_frames=2)
    torch.cuda.synchronize()
    ctx.motion_skip_device(d_luma.data_ptr() + sb * origin, sb, stride, fstride, 2, d_merge.data_ptr(), out.data_ptr() + GUARD, qp=qp, max_range=max_range)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:GUARD] == CANARY).all() and (h[GUARD + n:] == CANARY).all(), "a guard around the output was written"
    got = h[GUARD:GUARD + n].copy().view(KDT).reshape(qc.CTUS, 85)
    flags = check(got, quant_golden, bd, r, qi, merges[r], (dtype.__name__, bd, max_range, qp))
    # both outcomes of bit 0 at every QP but the ends, where the clip has one only
    assert (qp == 0 or (flags & 1).any()) and (qp == 51 or not (flags & 1).all())
    ctx.close()


def test_the_host_form_gives_the_references_numbers(torch_cuda, quant_golden):
    """fhevc_motion_skip: the quantiser's numbers computed by fhevc_skip_quant() on the host path"""
    bd, max_range = 10, 16
    pics, merges = clip(quant_golden, bd)
    r = qc.RANGES.index(max_range)
    (rb, org, stride), (cb, _, _) = pel(pics[0]), pel(pics[1])
    ctx = capi.Context(qc.W, qc.H, bd)
    seen = set()
    for qi, qp in enumerate(qc.NODE_QPS):
        got = ctx.motion_skip(cb, rb, merges[r], org, stride, qp=qp, max_range=max_range)
        seen |= set(check(got, quant_golden, bd, r, qi, merges[r], ("host", qp)).tolist())
    assert seen == {0, 1, 3}
    ctx.close()
