"""The C-ABI surface of the intra stage of P pictures and of the tree decision that takes its costs (no GPU needed: the library loads without one for
context-free functions): the 16-byte fhevc_intra_p_node in the header and in the Python mirror, the six entry points' signatures and exports, the header's
text for the new section and timing slot 27, calls rejected before a device is touched (fhevc_kernel_timing with a NULL context refuses slots 26, 27 and 28
alike: a context cannot exist without a GPU, so which slots the table knows is tests/test_gpu_intra_p.py's to show), and the host twins
fhevc_intra_p_picture and fhevc_p_tree_select_intra against the Python restatement of tests/intra_p_ref.py on the draw: every band, first4 NULL, pointers
4 bytes off, every combination of NULL outputs of the tree, and nothing written by a rejected call."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import intra_p_ref as ip
import p_tree_ref as pt
from fasthevc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fhevc_intra_p_device": 9, "fhevc_intra_p": 5, "fhevc_intra_p_picture": 8, "fhevc_p_tree_select_intra": 11, "fhevc_p_tree_select_intra_device": 14,
       "fhevc_p_tree_intra_frame": 15}
CANARY = 0xA5


def _header():
    return open(os.path.join(ROOT, "include", "fasthevc.h")).read()


def offset_copy(a, offset):
    """the bytes of `a` in a fresh buffer, starting `offset` bytes behind a 16-byte boundary -> (the buffer, the address)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = np.zeros(raw.size + 48, np.uint8)
    at = (-buf.ctypes.data) % 16 + offset
    buf[at:at + raw.size] = raw
    return buf, buf.ctypes.data + at


def host_stage(first, first4, W, H, qp, rows, in_offset=0, out_offset=0):
    """fhevc_intra_p_picture -> (rc, records [band CTUs, 85] or None when rejected); the output lies between canaries, which are checked"""
    lib = capi.load_library()
    n = first.size // 85 if first is not None else 1
    held = [None if a is None else offset_copy(a, in_offset) for a in (first, first4)]
    out = np.full(n * 85 * 16 + 64, CANARY, np.uint8)
    at = (-out.ctypes.data) % 16 + 16 + out_offset
    rc = lib.fhevc_intra_p_picture(W, H, rows[0], rows[1], qp, held[0][1] if held[0] else None, held[1][1] if held[1] else None, out.ctypes.data + at)
    assert (out[:at] == CANARY).all() and (out[at + n * 85 * 16:] == CANARY).all(), "a canary around the output was written"
    if rc != capi.OK:
        assert (out == CANARY).all(), "a rejected call wrote"
        return rc, None
    return rc, out[at:at + n * 85 * 16].copy().view(ip.IDT).reshape(n, 85)


def host_tree(shapes, merge, skip, mask, intra, vw, vh, rule, want=(True, True, True), offset=0):
    """fhevc_p_tree_select_intra on one CTU -> (rc, depth_min, depth_max, records), None for an output not asked for; outputs between canaries"""
    lib = capi.load_library()
    bufs = [np.full(n + 32, CANARY, np.uint8) for n in (256, 256, 85 * 16)]
    held = [None if a is None else offset_copy(a, offset) for a in (shapes, merge, skip, intra)]
    ptr = [None if h is None else h[1] for h in held]
    rc = lib.fhevc_p_tree_select_intra(ptr[0], ptr[1], ptr[2], mask, ptr[3], vw, vh, C.byref(rule) if rule is not None else None,
                                       *[b.ctypes.data + 16 if w else None for b, w in zip(bufs, want)])
    for b, w in zip(bufs, want):
        assert (b[:16] == CANARY).all() and (b[-16:] == CANARY).all(), "a canary around an output was written"
        if not w or rc != capi.OK:
            assert (b == CANARY).all(), "an output that was not asked for, or of a rejected call, was written"
    out = [b[16:-16].copy() if w else None for b, w in zip(bufs, want)]
    if out[2] is not None:
        out[2] = out[2].view(capi.TREE_DTYPE)
    return (rc, *out)


def test_struct_size_and_offsets():
    d = capi.INTRA_P_DTYPE
    assert d.itemsize == 16 and d.names == ("satd_best", "cost_best", "modes", "part", "pad")
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 12, 13] and d.fields["modes"][0].shape == (4,) and d.fields["pad"][0].shape == (3,)
    assert capi.TREE_INTRA == 1 == ip.INTRA and capi.TREE_DTYPE.fields["pad"][1] == 14
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fhevc_intra_p_node\s*;", _header())
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t satd_best", "uint32_t cost_best", "uint8_t modes[4]", "uint8_t part", "uint8_t pad[3]"]
    internal = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_internal.h")).read()
    assert "static_assert(sizeof(FhevcIntraPNode) == 16" in internal and "__host__ __device__ inline uint32_t fhevc_intra_p_price" in internal
    api = open(os.path.join(ROOT, "fasthevc_amd", "csrc", "fhevc_motion_api.hip")).read()
    assert "offsetof(fhevc_intra_p_node, cost_best) == 4" in api and "offsetof(fhevc_intra_p_node, part) == 12" in api


def test_header_python_mirror_and_exports():
    h = _header()
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym, nargs in NEW.items():
        m = re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h)
        assert m and len(strip(m.group(1)).split(",")) == nargs, sym
        assert sym in capi.SYMBOLS
    for sym in ("fhevc_intra_p_picture", "fhevc_p_tree_select_intra"):
        assert "fhevc_ctx" not in re.search(rf"\bint\s+{sym}\s*\(([^;]*)\);", h).group(1)
    for phrase in ("27 = the intra candidate costs", "26 is not a slot", "any number above 27", "Timed under slot 27", "TEncCu.cpp:797-816", "TEncCu.cpp:799-804",
                   "2 for mode 0, 3 for modes 1 and 26, 6 for every other byte value", "STRICTLY smaller", "the calm gate", "bit 0 of\n * byte 14",
                   "reconstructed neighbours", "the RD search behind HM's candidate list", "chroma, PCM", "The encoder hook does not consume this output",
                   "the skip flag, the pred-mode flag and the part mode", "INTEGER price of the first pass's winner",
                   # the slot text the earlier tests look for is still there
                   "24 is not a slot", "25 = the re-pricing", "22 is not a slot", "17 = the P-picture tree decision"):
        assert phrase in h, phrase
    sig = inspect.signature(capi.Context.intra_p_device)
    assert list(sig.parameters) == ["self", "num_pictures", "d_first", "d_first4", "d_out", "rows", "stream", "qp"]
    sig = inspect.signature(capi.Context.p_tree_select_intra_device)
    assert list(sig.parameters) == ["self", "d_shapes", "d_merge", "d_skip", "skip_mask", "d_intra", "num_pictures", "d_depth_min", "d_depth_max", "d_tree", "rows",
                                    "stream", "rule"]
    assert all(hasattr(capi, n) for n in ("p_tree_select_intra", "intra_p_picture")) and all(hasattr(capi.Context, n) for n in ("intra_p", "p_tree_intra_frame"))
    assert os.path.exists(capi.LIB_PATH), "HIP library not built (run __graft_entry__.build())"
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    lib = capi.load_library()
    for sym, nargs in NEW.items():
        assert re.search(rf"\bT {sym}\b", exported), sym
        assert len(getattr(lib, sym).argtypes) == nargs, sym


def test_rejected_without_a_device_and_the_timing_slots():
    lib = capi.load_library()
    assert lib.fhevc_intra_p_device(None, 1, 0, 1, 32, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_intra_p(None, 32, None, None, None) == capi.E_INVALID
    assert lib.fhevc_p_tree_select_intra_device(None, None, None, None, 1, None, 1, 0, 1, None, None, None, None, None) == capi.E_INVALID
    assert lib.fhevc_p_tree_intra_frame(None, None, None, 64, 32, 8, 0, None, None, 3, None, None, None, None, None) == capi.E_INVALID
    for slot in (26, 27, 28):      # the NULL context's refusal, whatever the slot: the slot table itself needs a context, and so a GPU
        assert lib.fhevc_kernel_timing(None, slot, 0, None, None) == capi.E_INVALID


def test_host_stage_rejected_calls_write_nothing():
    d = ip.draw((100, 76))
    first, first4 = d["first"][0], d["first4"][0]
    ok = lambda **kw: host_stage(kw.get("first", first), kw.get("first4", first4), kw.get("W", 100), kw.get("H", 76), kw.get("qp", 32), kw.get("rows", (0, 2)),
                                 kw.get("in_offset", 0), kw.get("out_offset", 0))[0]
    assert ok() == capi.OK and ok(first4=None) == capi.OK and ok(qp=0) == capi.OK and ok(qp=51) == capi.OK
    for change in (dict(first=None), dict(qp=-1), dict(qp=52), dict(rows=(-1, 2)), dict(rows=(0, 3)), dict(rows=(2, 1)), dict(W=7), dict(H=7), dict(in_offset=2),
                   dict(in_offset=1), dict(out_offset=2), dict(out_offset=3)):
        assert ok(**change) == capi.E_INVALID, change             # host_stage asserts that nothing was written
    lib = capi.load_library()
    assert lib.fhevc_intra_p_picture(100, 76, 0, 2, 32, first.ctypes.data, None, None) == capi.E_INVALID


@pytest.mark.parametrize("size", ip.DRAW_SIZES)
def test_host_stage_equals_the_restatement_on_the_draw(size):
    W, H = size
    d = ip.draw(size)
    cw, ch = (W + 63) // 64, (H + 63) // 64
    bands = [(a, b) for a in range(ch + 1) for b in range(a, ch + 1)]
    for p in range(ip.DRAW_PICTURES):
        for rows in (bands if p < 2 else [bands[p % len(bands)], (0, ch)]):
            sl = slice(rows[0] * cw, rows[1] * cw)
            for f4, exp in ((d["first4"], d["out"]), (None, d["out_no4"])):
                rc, got = host_stage(d["first"][p, sl], None if f4 is None else f4[p, sl], W, H, ip.DRAW_QP, rows)
                assert rc == capi.OK
                if rows[0] == rows[1]:
                    continue                                   # an empty band: nothing written (host_stage's canaries cover the whole buffer)
                ip.same(got, exp[p, sl], (p, rows, f4 is None))
    # pointers 4, 8 and 12 bytes off a 16-byte boundary, inputs and output independently: the same bytes
    for in_off, out_off in ((4, 0), (0, 4), (8, 12), (12, 8), (4, 4)):
        rc, got = host_stage(d["first"][0], d["first4"][0], W, H, ip.DRAW_QP, (0, ch), in_off, out_off)
        assert rc == capi.OK
        ip.same(got, d["out"][0], (in_off, out_off))
    # another QP: the draw's records are legal input at any
    for qp in (0, 51):
        rc, got = host_stage(d["first"][1], d["first4"][1], W, H, qp, (0, ch))
        ip.same(got, ip.stage(d["first"][1:2], d["first4"][1:2], W, H, qp)[0], qp)
    # the wrapper
    ip.same(capi.intra_p_picture(d["first"][2], d["first4"][2], W, H, qp=ip.DRAW_QP), d["out"][2], "capi.intra_p_picture")


@pytest.mark.parametrize("size", ip.DRAW_SIZES)
def test_host_tree_equals_the_restatement_on_the_draw(size):
    W, H = size
    d = ip.draw(size)
    combos = [w for w in itertools.product((True, False), repeat=3) if any(w)]
    assert len(combos) == 7
    names = list(d["rules"])
    n = d["shapes"].shape[1]
    for p in range(ip.DRAW_PICTURES):
        rname, mask = names[p % 4], (p // 4 + p) % 4
        erec, emin, emax = ip.draw_tree(size, rname, mask)
        for c in range(n):
            vw, vh = pt.valid_size(c, W, H)
            for want in (combos if (p + c) % 5 == 0 else [combos[(p + c) % 7]]):
                rc, dmin, dmax, rec = host_tree(d["shapes"][p, c], d["merge"][p, c], d["skip"][p, c], mask, d["intra"][p, c], vw, vh, d["rules"][rname], want,
                                                offset=4 * ((p + c) % 4))
                assert rc == capi.OK
                assert dmin is None or np.array_equal(dmin, emin[p, c]), (p, c, mask)
                assert dmax is None or np.array_equal(dmax, emax[p, c]), (p, c, mask)
                if rec is not None:
                    ip.same_tree(rec, erec[p, c], (p, c, mask))
    # every mask and rule on one picture, through the wrapper
    for rname, mask in itertools.product(names, range(4)):
        erec, emin, emax = (a[:1] for a in ip.tree_select(d["shapes"][:1], d["merge"][:1], d["skip"][:1], mask, d["intra"][:1], W, H, rule=d["rules"][rname]))
        gmin, gmax, grec = capi.p_tree_select_intra(d["shapes"][0], d["merge"][0], d["skip"][0], mask, d["intra"][0], W, H, rule=d["rules"][rname], with_tree=True)
        ip.same_tree(grec, erec[0], (rname, mask))
        assert np.array_equal(gmin, emin[0]) and np.array_equal(gmax, emax[0])
    # all-MARK intra records: byte for byte fhevc_p_tree_select_skip
    blank = ip.all_mark(d["intra"])
    for mask in (0, 3):
        a = capi.p_tree_select_intra(d["shapes"][3], d["merge"][3], d["skip"][3], mask, blank[3], W, H, rule=d["rules"]["r2"], with_tree=True)
        b = capi.p_tree_select_skip(d["shapes"][3], d["merge"][3], d["skip"][3], mask, W, H, rule=d["rules"]["r2"], with_tree=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), mask


def test_host_tree_rejected_calls_write_nothing():
    d = ip.draw((100, 76))
    s, m, k, i = (d[n][0, 0] for n in ("shapes", "merge", "skip", "intra"))
    r = capi.p_tree_rule_default()
    ok = lambda **kw: host_tree(kw.get("shapes", s), kw.get("merge", m), kw.get("skip", k), kw.get("mask", 3), kw.get("intra", i), kw.get("vw", 64), kw.get("vh", 64),
                                kw.get("rule", r), kw.get("want", (True, True, True)))[0]
    assert ok() == capi.OK
    for change in (dict(intra=None), dict(skip=None), dict(mask=-1), dict(mask=4), dict(merge=None), dict(shapes=None), dict(rule=None), dict(vw=7), dict(vh=65),
                   dict(want=(False, False, False)), dict(rule=capi.p_tree_rule(split_q8=[0, 65536, 0])), dict(rule=capi.p_tree_rule(split_cost=[-1, 0, 0]))):
        assert ok(**change) == capi.E_INVALID, change
