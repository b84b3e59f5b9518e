"""Config 4 (P slices) on the MI355X against what the REFERENCE itself returned, with no restatement in between: the integer searches in SAD mode
(k_motion.hip, k_motion_pu.hip, k_motion_pu_small.hip) against tests/golden/ref_pattern_search_pu.npz (TEncSearch::xPatternSearch on w x h
patterns), the quarter-sample refinements (k_motion_refine.hip, k_motion_refine_pu.hip) against tests/golden/ref_frac_search.npz
(TEncSearch::xPatternSearchFracDIF with UseHADME, fed the file's integer vectors).  Goldens only (tests/motion_golden.py), through the C ABI;
every valid entry of the files' five CTUs, field by field, the marker where the files hold -1, and the count of what was compared asserted.
The searches' SATD mode at integer positions is this build's own choice, has no counterpart in the reference and stays with its restatement
(test_gpu_motion_pu.py, test_gpu_motion_pu_small.py)."""
import numpy as np
import pytest

import motion_golden as mg
from fasthevc_amd import capi
from motion_gpu_helpers import Guarded, pel, to_dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

QDT = capi.MOTION_QPEL_DTYPE
PER = {"nodes": capi.NODES_PER_CTU, "pu": capi.PUS_PER_CTU, "small": capi.PUS_SMALL_PER_CTU}
PER_CASE = {"nodes": 267, "pu": 348, "small": 1224}   # valid entries of the five CTUs: whole, 48 wide, whole, 16 tall, 48 x 16


@pytest.fixture(scope="module")
def search_cases():
    return mg.search_cases()


@pytest.fixture(scope="module")
def frac_cases():
    return mg.frac_cases()


def context(c, **kw):
    ctx = capi.Context(c.W, c.H, c.bd, **kw)
    ctx.set_motion_distortion("sad")     # the searches' distortion; the refinement is Hadamard whatever this says
    assert ctx.num_ctus == c.num_ctus
    return ctx


def test_integer_searches_equal_the_reference(search_cases):
    done = dict.fromkeys(mg.FAMILIES, 0)
    for c in search_cases:
        (rb, org, stride), (cb, _, _) = pel(c.ref), pel(c.cur)
        ctx = context(c)
        nodes, pus = ctx.motion_search_pu(cb, rb, org, stride, qp=c.qp, search_range=c.R, with_nodes=True)
        small = ctx.motion_search_pu_small(cb, rb, org, stride, qp=c.qp, search_range=c.R)
        for fam, got in (("nodes", nodes), ("pu", pus), ("small", small)):
            done[fam] += mg.same(got[c.ctus], c.records(fam), (c, fam))
        mg.same(ctx.motion_search(cb, rb, org, stride, qp=c.qp, search_range=c.R)[c.ctus], c.records("nodes"), (c, "the square search"))
        ctx.close()
    assert done == mg.SEARCH_COUNTS


def test_refinements_equal_the_reference(frac_cases):
    done = dict.fromkeys(mg.FAMILIES, 0)
    for c in frac_cases:
        (rb, org, stride), (cb, _, _) = pel(c.ref), pel(c.cur)
        ctx = context(c)
        ins = {fam: c.inputs(fam, seed=c.k) for fam in mg.FAMILIES}
        got = {"nodes": ctx.motion_refine(cb, rb, ins["nodes"], org, stride, qp=c.qp, max_range=c.R)}
        got["pu"], got["small"] = ctx.motion_refine_pu(cb, rb, org, stride, qp=c.qp, max_range=c.R, pus=ins["pu"], pus_small=ins["small"])
        for fam in mg.FAMILIES:
            done[fam] += mg.same(got[fam][c.ctus], c.records(fam), (c, fam))
        # one family at a time: the other comes back as None
        only, none = ctx.motion_refine_pu(cb, rb, org, stride, qp=c.qp, max_range=c.R, pus=ins["pu"])
        assert none is None and mg.same(only[c.ctus], c.records("pu"), (c, "pu alone")) == PER_CASE["pu"]
        none, only = ctx.motion_refine_pu(cb, rb, org, stride, qp=c.qp, max_range=c.R, pus_small=ins["small"])
        assert none is None and mg.same(only[c.ctus], c.records("small"), (c, "small alone")) == PER_CASE["small"]
        ctx.close()
    assert done == mg.FRAC_COUNTS


def byte_planes(torch, c):
    """the case's two pictures as one device batch of uint8 planes without margins (reference first): sample_bytes 1, stride W, frame stride W H"""
    assert c.bd == 8
    return to_dev(torch, np.stack([c.ref, c.cur]).astype(np.uint8)), c.W, c.W * c.H


def test_device_forms_on_uint8_planes_integer_searches(search_cases, torch_cuda):
    """the 8-bit cases again through the *_device forms on byte planes (the byte load path of the tile load, the 8-byte staging load), the outputs
    between canaries"""
    torch = torch_cuda
    cases = [c for c in search_cases if c.bd == 8]
    done = dict.fromkeys(mg.FAMILIES, 0)
    for c in cases:
        d_luma, stride, fs = byte_planes(torch, c)
        ctx = context(c, max_frames=2)
        g = {fam: Guarded(torch, c.num_ctus * PER[fam] * 16) for fam in mg.FAMILIES}
        square = Guarded(torch, c.num_ctus * PER["nodes"] * 16)
        torch.cuda.synchronize()
        ctx.motion_search_pu_device(d_luma.data_ptr(), 1, stride, fs, 2, g["pu"].ptr, d_nodes=g["nodes"].ptr, qp=c.qp, search_range=c.R)
        ctx.motion_search_pu_small_device(d_luma.data_ptr(), 1, stride, fs, 2, g["small"].ptr, qp=c.qp, search_range=c.R)
        ctx.motion_search_device(d_luma.data_ptr(), 1, stride, fs, 2, square.ptr, qp=c.qp, search_range=c.R)
        torch.cuda.synchronize()
        for fam in mg.FAMILIES:
            done[fam] += mg.same(g[fam].result((c.num_ctus, PER[fam]))[c.ctus], c.records(fam), (c, fam))
        mg.same(square.result((c.num_ctus, PER["nodes"]))[c.ctus], c.records("nodes"), (c, "the square search"))
        ctx.close()
    assert len(cases) >= 1 and done == {fam: len(cases) * n for fam, n in PER_CASE.items()}


def test_device_forms_on_uint8_planes_refinements(frac_cases, torch_cuda):
    torch = torch_cuda
    cases = [c for c in frac_cases if c.bd == 8]
    done = dict.fromkeys(mg.FAMILIES, 0)
    for c in cases:
        d_luma, stride, fs = byte_planes(torch, c)
        ctx = context(c, max_frames=2)
        d_in = {fam: to_dev(torch, c.inputs(fam, seed=100 + c.k)) for fam in mg.FAMILIES}
        g = {fam: Guarded(torch, c.num_ctus * PER[fam] * 16) for fam in mg.FAMILIES}
        torch.cuda.synchronize()
        ctx.motion_refine_device(d_luma.data_ptr(), 1, stride, fs, 2, d_in["nodes"].data_ptr(), g["nodes"].ptr, qp=c.qp, max_range=c.R)
        ctx.motion_refine_pu_device(d_luma.data_ptr(), 1, stride, fs, 2, d_in["pu"].data_ptr(), g["pu"].ptr, d_in["small"].data_ptr(), g["small"].ptr, qp=c.qp, max_range=c.R)
        torch.cuda.synchronize()
        for fam in mg.FAMILIES:
            done[fam] += mg.same(g[fam].result((c.num_ctus, PER[fam])).view(QDT)[c.ctus], c.records(fam), (c, fam))
        ctx.close()
    assert len(cases) >= 1 and done == {fam: len(cases) * n for fam, n in PER_CASE.items()}
