"""The C-ABI surface of the re-pricing against neighbour predictors (no GPU needed: the library loads without one for context-free functions): the four
entry points in the header, in the Python mirror and among the exports, the header's normative phrases with their HM lines, calls rejected before a device
is touched, timing slots 25 and 24, and the host twin fhevc_motion_amvp_picture against the Python restatement of tests/motion_amvp_ref.py: the draw on two
pictures, three bit depths, six QPs and bands as slices, every combination of NULL arrays, arrays 4 bytes off a 16-byte boundary, outputs between canaries."""
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import motion_amvp_ref as ar
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_motion_amvp_device": 15, "fhevc_motion_amvp": 11, "fhevc_motion_amvp_picture": 15, "fhevc_p_tree_amvp_frame": 13}
FAMILIES = ("nodes", "pu", "small")
CANARY = 0xA5
QPS = (0, 4, 22, 32, 40, 51)


def host_call(W, H, bd, rows, qp, ins, want_out=(True,) * 3, want_mvp=(True,) * 3, offset=0):
    """fhevc_motion_amvp_picture on arrays `offset` bytes behind a 16-byte boundary, outputs between canaries -> (rc, records x 3, predictor records x 3), None
    for an array not asked for; a rejected call must leave every output byte alone"""
    lib = capi.load_library()
    cw = (W + 63) // 64
    n = max(0, rows[1] - rows[0]) * cw
    held, bufs, ptrs = [], [], []
    for a in ins:
        if a is None:
            ptrs.append(None)
            continue
        raw = np.zeros(a.size * 16 + 32, np.uint8)
        at = (-raw.ctypes.data) % 16 + offset
        raw[at:at + a.size * 16] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        held.append(raw)
        ptrs.append(raw.ctypes.data + at)
    for want, size in ((want_out, 16), (want_mvp, 8)):
        for f, w in zip(FAMILIES, want):
            raw = np.full(n * ar.PER[f] * size + 64, CANARY, np.uint8)
            at = (-raw.ctypes.data) % 16 + 16 + offset
            bufs.append((raw, at, n * ar.PER[f] * size, w))
            ptrs.append(raw.ctypes.data + at if w else None)
    rc = lib.fhevc_motion_amvp_picture(W, H, bd, rows[0], rows[1], qp, *ptrs)
    out = []
    for (raw, at, size, w), dt, f in zip(bufs, (ar.QDT,) * 3 + (ar.VDT,) * 3, FAMILIES * 2):
        assert (raw[:at] == CANARY).all() and (raw[at + size:] == CANARY).all(), "a canary around an output was written"
        if not w or rc != capi.OK:
            assert (raw == CANARY).all(), "an output that was not asked for, or of a rejected call, was written"
        out.append(raw[at:at + size].copy().view(dt).reshape(n, ar.PER[f]) if w and rc == capi.OK else None)
    return (rc,) + tuple(out)


def test_header_python_mirror_and_exports():
    h = open(os.path.join(ROOT, "include", "fasthevc.h")).read()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym, nargs in NEW.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m and len(strip(m.group(1)).split(",")) == nargs, sym
        assert sym in capi.SYMBOLS
    assert "fhevc_ctx" not in re.search(r"\bint\s+fhevc_motion_amvp_picture\s*\(([^;]*)\);", h).group(1)
    assert "d_luma" not in re.search(r"\bint\s+fhevc_motion_amvp_device\s*\(([^;]*)\);", h).group(1)          # it takes no planes
    for phrase in ("TComDataCU.cpp:2578-2716", "TEncSearch.cpp:3028", ":3566-3615", ":2603-2619", ":2621-2632", ":2634-2645", ":2647-2653", ":2710-2714",
                   "TComRdCost.h:166-174", "xGetMvpIdxBits", "DEPARTURE", "takes the lower index", "no second-PU exclusion", "min(satd_best + c[bits_idx], 0xFFFFFFFE)",
                   "67 entries", "Timed under slot 25", "25 = the re-pricing", "24 is not a slot", "Table entries 39..66 rest on the formula"):
        assert phrase in h, phrase
    assert capi.MOTION_MVP_DTYPE.itemsize == 8 and capi.MOTION_MVP_DTYPE.names == ("px", "py", "idx", "num_spatial", "src", "bits")
    assert list(inspect.signature(capi.Context.motion_amvp).parameters) == ["self", "nodes", "pus", "pus_small", "qp", "with_records", "with_mvp"]
    assert list(inspect.signature(capi.Context.motion_amvp_device).parameters) == ["self", "num_frames", "d_nodes", "d_pus", "d_pus_small", "d_out_nodes", "d_out_pus",
                                                                                  "d_out_pus_small", "d_mvp_nodes", "d_mvp_pus", "d_mvp_pus_small", "rows", "stream", "qp"]
    assert list(inspect.signature(capi.motion_amvp_picture).parameters) == ["nodes", "pus", "pus_small", "width", "height", "bit_depth", "qp", "rows", "with_records", "with_mvp"]
    assert hasattr(capi.Context, "p_tree_amvp_frame")
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym


def test_rejected_without_a_device_and_the_timing_slots():
    lib = capi.load_library()
    assert lib.fhevc_motion_amvp_device(None, 2, 0, 1, 32, *([None] * 10)) == capi.E_INVALID
    assert lib.fhevc_motion_amvp(None, 32, *([None] * 9)) == capi.E_INVALID
    assert lib.fhevc_p_tree_amvp_frame(None, None, None, 64, 32, 8, 0, None, None, None, None, None, None) == capi.E_INVALID
    for slot in (25, 24, 26):
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID


def test_host_twin_rejects_and_leaves_the_outputs_alone():
    W, H = ar.DRAW_W, ar.DRAW_H
    ins = list(ar.random_draw(0))
    assert host_call(W, H, 8, (0, 3), 32, ins)[0] == capi.OK
    for kw in (dict(W=7), dict(H=7), dict(bd=7), dict(bd=13), dict(qp=-1), dict(qp=52), dict(rows=(-1, 3)), dict(rows=(0, 4)), dict(rows=(2, 1))):
        a = dict(dict(W=W, H=H, bd=8, rows=(0, 3), qp=32), **kw)
        assert host_call(a["W"], a["H"], a["bd"], a["rows"], a["qp"], ins)[0] == capi.E_INVALID, kw
    assert host_call(W, H, 8, (0, 3), 32, [None] + ins[1:])[0] == capi.E_INVALID                        # the nodes are always required
    assert host_call(W, H, 8, (0, 3), 32, ins, (False,) * 3, (False,) * 3)[0] == capi.E_INVALID         # at least one output
    # a family's outputs need that family's input
    assert host_call(W, H, 8, (0, 3), 32, [ins[0], None, ins[2]], (True, True, True), (False,) * 3)[0] == capi.E_INVALID
    assert host_call(W, H, 8, (0, 3), 32, [ins[0], ins[1], None], (False,) * 3, (False, False, True))[0] == capi.E_INVALID
    # the empty band: accepted, nothing written (host_call checks the canaries of zero-length outputs)
    assert host_call(W, H, 8, (1, 1), 32, [a[:0] for a in ins])[0] == capi.OK


def test_host_twin_equals_the_restatement_on_the_draw():
    ins, exp, _ = ar.draw_batch()
    for d in range(0, ar.DRAWS, 7):
        got = host_call(ar.DRAW_W, ar.DRAW_H, 8, (0, 3), ar.DRAW_QP, [ins[f][d] for f in FAMILIES])
        assert got[0] == capi.OK
        for i, f in enumerate(FAMILIES):
            ar.same(got[1 + i], exp[f][0][d], (d, f))
            ar.same(got[4 + i], exp[f][1][d], (d, f, "mvp"))
    # ... and through the Python mirror
    got = capi.motion_amvp_picture(ins["nodes"][1], ins["pu"][1], ins["small"][1], ar.DRAW_W, ar.DRAW_H, qp=ar.DRAW_QP, with_mvp=True)
    for i, f in enumerate(FAMILIES):
        ar.same(got[i], exp[f][0][1], f)
        ar.same(got[3 + i], exp[f][1][1], f)


@pytest.mark.parametrize("W,H", [(168, 152), (200, 136)])
def test_host_twin_bit_depths_qps_and_bands(W, H):
    """8 / 10 / 12 bit, six QPs, the whole picture and every band of it as a slice: candidates never cross a band"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    rng = np.random.default_rng(W)
    full = [ar.random_records(rng, (cw * ch, ar.PER[f])) for f in FAMILIES]
    bands = [(0, ch)] + [(b, e) for b in range(ch) for e in range(b + 1, ch + 1) if (b, e) != (0, ch)]
    for (bd, qp), rows in zip(itertools.cycle(zip((8, 10, 12, 8, 10, 12), QPS)), bands + bands):
        cut = [a[rows[0] * cw:rows[1] * cw] for a in full]
        exp = ar.expected_all(W, H, *cut, qp, rows=rows)
        got = host_call(W, H, bd, rows, qp, cut)
        assert got[0] == capi.OK
        for i, f in enumerate(FAMILIES):
            ar.same(got[1 + i], exp[f][0], (bd, qp, rows, f))
            ar.same(got[4 + i], exp[f][1], (bd, qp, rows, f, "mvp"))
    # a band is a slice: the first CTU row of a band has no candidate above it
    rows = (1, ch)
    exp = ar.expected_all(W, H, *[a[cw:] for a in full], 32, rows=rows)
    whole = ar.expected_all(W, H, *full, 32)
    assert any((exp[f][1][:cw] != whole[f][1][cw:2 * cw]).any() for f in FAMILIES)


def test_host_twin_every_null_combination_and_pointers_off_16():
    ins, exp, _ = ar.draw_batch()
    one = [ins[f][2] for f in FAMILIES]
    ok = 0
    for have in itertools.product((True, False), repeat=2):
        given = [one[0]] + [a if h else None for a, h in zip(one[1:], have)]
        for want in itertools.product((True, False), repeat=6):
            legal = any(want) and all(g is not None or not (want[i] or want[3 + i]) for i, g in enumerate(given))
            got = host_call(ar.DRAW_W, ar.DRAW_H, 10, (0, 3), ar.DRAW_QP, given, want[:3], want[3:], offset=4 * (ok % 4))
            assert got[0] == (capi.OK if legal else capi.E_INVALID), (have, want)
            if legal:
                ok += 1
                for i, f in enumerate(FAMILIES):
                    for j, g in ((0, got[1 + i]), (1, got[4 + i])):
                        if g is not None:
                            ar.same(g, exp[f][j][2], (have, want, f, j))
    assert ok == 63 + 15 + 15 + 3
    for offset in (4, 8, 12):
        got = host_call(ar.DRAW_W, ar.DRAW_H, 8, (0, 3), ar.DRAW_QP, one, offset=offset)
        for i, f in enumerate(FAMILIES):
            ar.same(got[1 + i], exp[f][0][2], (offset, f))
            ar.same(got[4 + i], exp[f][1][2], (offset, f))
