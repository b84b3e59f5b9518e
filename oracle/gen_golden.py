#!/usr/bin/env python3
"""Generate tests/golden/ref_vectors.npz by running the REFERENCE's own functions
(oracle/_ref/libhmref.so = objects compiled from /root/reference + oracle/ref_harness.cpp).

Run in the build container only (needs /root/reference):  make -C oracle ref && python oracle/gen_golden.py
(--bit-depths-only: tests/golden/ref_bit_depths.npz alone, bit_depths_golden;
 --motion-pu-only: tests/golden/ref_pattern_search_pu.npz and ref_frac_search.npz alone, motion_pu_golden)
The fixture holds inputs and expected outputs (data), never reference source.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle_py as op  # noqa: E402
from fasthevc_amd import frames  # noqa: E402


def main():
    ref = op.load_ref()
    out = {"hm_version": np.frombuffer(ref.href_version(), np.uint8)}
    rng = np.random.default_rng(20261004)

    # --- scan tables (A14)
    r2z = np.zeros(256, np.uint32)
    z2r = np.zeros(256, np.uint32)
    ref.href_scan_tables(r2z, z2r)
    out["raster_to_zscan"], out["zscan_to_raster"] = r2z, z2r

    # --- SATD (A5): calcHAD and xGetHADs, 8- and 10-bit, square and rectangular
    shapes = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (8, 4), (4, 8), (16, 8), (8, 16), (32, 8), (16, 4), (2, 2), (6, 6)]
    satd_a, satd_b, satd_meta, satd_calc, satd_get = [], [], [], [], []
    for bd in (8, 10):
        for (w, h) in shapes:
            for rep in range(3):
                hi = (1 << bd) - 1
                if rep == 2:  # extremes: exercises the largest intermediates
                    a = rng.choice(np.array([0, hi], np.int16), size=(64, 64))
                    b = rng.choice(np.array([0, hi], np.int16), size=(64, 64))
                else:
                    a = rng.integers(0, hi + 1, size=(64, 64)).astype(np.int16)
                    b = np.clip(a + rng.normal(0, 12 * (1 << (bd - 8)), size=(64, 64)), 0, hi).astype(np.int16)
                g = ref.href_get_hads(bd, op.ptr(a), 64, op.ptr(b), 64, w, h)
                c = ref.href_calc_had(bd, op.ptr(a), 64, op.ptr(b), 64, w, h) if (w % 4 == 0 and h % 4 == 0) else 0xFFFFFFFF
                satd_a.append(a); satd_b.append(b); satd_meta.append((bd, w, h)); satd_calc.append(c); satd_get.append(g)
    out["satd_a"] = np.stack(satd_a); out["satd_b"] = np.stack(satd_b)
    out["satd_meta"] = np.array(satd_meta, np.int32)
    out["satd_calchad"] = np.array(satd_calc, np.uint32); out["satd_gethads"] = np.array(satd_get, np.uint32)

    # --- source Hadamard (A6): single blocks + per-CTU sums of the pinned synthetic frames
    blk = rng.integers(0, 1024, size=(16, 8, 8)).astype(np.int16)
    out["islice_blocks"] = blk
    out["islice_expected"] = np.array([ref.href_had8x8_islice(op.ptr(np.ascontiguousarray(b)), 8) for b in blk], np.int32)
    for name, (w, h, bd) in {"t16_416x240_8": (416, 240, 8), "t16_416x240_10": (416, 240, 10), "t16_1920x1080_8": (1920, 1080, 8)}.items():
        luma = frames.texture16_luma(w, h)
        buf, org, stride = frames.to_pel_plane(luma, bd)
        flat = buf.reshape(-1)
        cw, ch = frames.ctu_grid(w, h)
        vals = np.zeros(cw * ch, np.int32)
        for cy in range(ch):
            for cx in range(cw):
                vals[cy * cw + cx] = ref.href_ctu_src_hadamard(op.ptr(flat, org + cy * 64 * stride + cx * 64), stride,
                                                               min(64, w - cx * 64), min(64, h - cy * 64))
        out["ctu_had_" + name] = vals

    # --- reference-sample fill (A7) on random availability patterns
    fr_roi, fr_flags, fr_n, fr_bd, fr_out = [], [], [], [], []
    for n in (4, 8, 16, 32, 64):
        for rep in range(6):
            bd = 8 if rep % 2 == 0 else 10
            pic = rng.integers(0, 1 << bd, size=(2 * n + 8, 2 * n + 8)).astype(np.int16)
            units = 2 * n // 4
            if rep == 0:
                flags = np.ones(2 * units + 1, np.uint8)
            elif rep == 1:
                flags = np.zeros(2 * units + 1, np.uint8)
            else:
                flags = (rng.random(2 * units + 1) < (0.3 + 0.2 * rep / 6)).astype(np.uint8)
                if rep == 5:
                    flags[:units] = 0  # nothing below/left available -> exercises the "search upward" padding
            roi = np.zeros((2 * n + 1) * (2 * n + 1), np.int16)
            stride = pic.shape[1]
            ref.href_fill_ref(bd, op.ptr(pic.reshape(-1), 4 * stride + 4), stride, flags, n, roi)
            full = np.zeros((129, 129), np.int16)
            full[:2 * n + 1, :2 * n + 1] = roi.reshape(2 * n + 1, 2 * n + 1)
            padded = np.zeros((136, 136), np.int16)
            padded[:pic.shape[0], :pic.shape[1]] = pic
            fl = np.zeros(65, np.uint8); fl[:flags.size] = flags
            fr_roi.append(padded); fr_flags.append(fl); fr_n.append(n); fr_bd.append(bd); fr_out.append(full)
    out["fill_pic"] = np.stack(fr_roi); out["fill_flags"] = np.stack(fr_flags)
    out["fill_n"] = np.array(fr_n, np.int32); out["fill_bd"] = np.array(fr_bd, np.int32); out["fill_out"] = np.stack(fr_out)

    # --- filter decision table (A7) and the 35 predictors (A8)
    out["use_filtered"] = np.array([[ref.href_use_filtered(m, n) for m in range(35)] for n in (4, 8, 16, 32, 64)], np.uint8)
    for n in (4, 8, 16, 32, 64):
        reps = 2 if n <= 32 else 1
        for rep in range(reps):
            bd = 8 if rep == 0 else 10
            line = np.clip(rng.integers(0, 1 << bd, size=4 * n + 1) * (0.5 + 0.5 * rng.random()), 0, (1 << bd) - 1).astype(np.int16)
            if rep == 1:
                line[::7] = (1 << bd) - 1  # saturating samples for the edge-filter clip
            roi = np.ascontiguousarray(op.ref_line_to_roi(line, n).reshape(-1))
            preds = np.zeros((35, n, n), np.int16)
            for m in range(35):
                p = np.zeros(n * n, np.int16)
                ref.href_pred_intra(roi, n, m, bd, p)
                preds[m] = p.reshape(n, n)
            out[f"pred_line_n{n}_bd{bd}"] = line
            out[f"pred_out_n{n}_bd{bd}"] = preds

    dst = os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_vectors.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    preanalyze_golden(ref)
    intra_lines_golden(ref)
    pattern_search_golden(ref)
    pattern_search_golden(ref, PATTERN_SEARCH_WIDE_CASES, "ref_pattern_search_wide.npz")
    pattern_search_golden(ref, PATTERN_SEARCH_WIDE10_CASES, "ref_pattern_search_wide10.npz")


PREANALYZE_CASES = (("texture16", 416, 240, 8, 3), ("hetero", 1000, 568, 10, 4), ("hetero", 64, 64, 8, 1))


def preanalyze_golden(ref):
    """TEncPreanalyzer::xPreanalyze outputs (N3) on the md5-pinned synthetic pictures: expected doubles only."""
    out = {"cases": np.array([f"{c[0]}:{c[1]}x{c[2]}:bd{c[3]}:d{c[4]}" for c in PREANALYZE_CASES])}
    for k, (content, w, h, bd, depth) in enumerate(PREANALYZE_CASES):
        luma = frames.texture16_luma(w, h) if content == "texture16" else frames.hetero_luma(w, h)
        buf, org, stride = frames.to_pel_plane(luma, bd)
        n = sum(((w + (64 >> d) - 1) // (64 >> d)) * ((h + (64 >> d) - 1) // (64 >> d)) for d in range(depth))
        act = np.zeros(n)
        avg = np.zeros(depth)
        assert ref.href_preanalyze(op.ptr(buf.reshape(-1), org), stride, w, h, bd, depth, act, avg) == n
        out[f"act{k}"], out[f"avg{k}"] = act, avg
        for range_, qp in ((6, 32), (12, 3), (4, 50)):  # TEncCu::xComputeQP on those activities (clips at both ends)
            q = np.zeros(n, np.int32)
            assert ref.href_aq_qp(op.ptr(buf.reshape(-1), org), stride, w, h, bd, depth, range_, qp, q) == n
            out[f"qp{k}_r{range_}_q{qp}"] = q.astype(np.int8)
    dst = os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_preanalyze.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


INTRA_LINE_CASES = (("hetero", 416, 240, 8, 32, (0, 1, 6, 7, 9, 13, 21, 24, 27)), ("texture16", 416, 240, 10, 27, (0, 6, 8, 20, 27)))


def intra_lines_golden(ref):
    """A7: unfiltered + smoothed reference lines from the reference's own initIntraPatternChType on live CUs (availability
    rule, substitution walk, [1 2 1] and strong smoothing), neighbours read from the original picture; and the reference's
    own xModeBitsIntra for the CU at the picture origin.  Expected outputs only."""
    import ctypes as C
    lib = op.bind_rdo(ref)
    lib.href_intra_lines.argtypes = [C.c_int] * 7 + [C.c_void_p, C.c_void_p]
    lib.href_mode_bits_origin.argtypes = [C.c_int] * 5 + [C.c_void_p]
    out = {"cases": np.array([f"{c[0]}:{c[1]}x{c[2]}:bd{c[3]}:qp{c[4]}" for c in INTRA_LINE_CASES])}
    for k, (content, w, h, bd, qp, ctus) in enumerate(INTRA_LINE_CASES):
        luma = frames.texture16_luma(w, h) if content == "texture16" else frames.hetero_luma(w, h)
        buf, org, stride = frames.to_pel_plane(luma, bd)
        if bd > 8:  # use the low bits too (the same recipe as the tests)
            m = org % stride
            buf[m:m + h, m:m + w] += np.random.default_rng(bd).integers(0, 1 << (bd - 8), (h, w)).astype(np.int16)
        op.rdo_encode(lib, buf, org, stride, w, h, bd, qp)  # live TComPic / TComDataCU objects for this geometry
        cw = (w + 63) // 64
        meta, unf, flt = [], [], []
        first = True
        for c in ctus:
            for depth in range(4):
                n = 64 >> depth
                for by in range(1 << depth):
                    for bx in range(1 << depth):
                        x0, y0 = (c % cw) * 64 + bx * n, (c // cw) * 64 + by * n
                        if x0 + n > w or y0 + n > h:
                            continue
                        a, b = np.zeros(4 * n + 1, np.int16), np.zeros(4 * n + 1, np.int16)
                        rc = lib.href_intra_lines(w, h, bd, c, depth, (by * n // 4) * 16 + bx * n // 4, 1 if first else 0, a.ctypes.data, b.ctypes.data)
                        assert rc == 4 * n + 1, rc
                        first = False
                        meta.append((c, depth, x0, y0, n)); unf.append(a); flt.append(b)
        out[f"meta{k}"] = np.array(meta, np.int32)
        out[f"unf{k}"] = np.concatenate(unf)
        out[f"flt{k}"] = np.concatenate(flt)
    bits = np.zeros((3, 4, 35), np.uint32)
    for i, qp in enumerate((22, 32, 37)):
        for depth in range(4):
            assert lib.href_mode_bits_origin(416, 240, 8, qp, depth, bits[i, depth].ctypes.data) == 35
    out["mode_bits_qp22_32_37"] = bits
    dst = os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_intra_lines.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")



PATTERN_SEARCH_CASES = (  # (bit depth, qp, range, clip seed, CTUs of the 7 x 4 grid of 416x240: corners, edges (32 wide / 48 tall), interior)
    (8, 38, 4, 15, (0, 3, 6, 10, 21, 27)),
    (10, 33, 3, 16, (8, 13, 20)),
    (8, 22, 8, 17, (9, 26)))


PATTERN_SEARCH_WIDE_CASES = (  # the same at HM's own SearchRange and two odd ones, 8 bit, clips with large motion: (.., clip seed, CTUs, speeds)
    (8, 32, 64, 31, (0, 9, 27), (21, -37)),
    (8, 27, 24, 32, (3, 13), (13, 9)),
    (8, 37, 33, 33, (6, 17, 24), (-30, 5)))


PATTERN_SEARCH_WIDE10_CASES = (  # round 4: the wide window ABOVE 8 bit (16-bit SAD kernel laid out for +-64, k_motion.hip): 10 and 12 bit, low bits populated
    (10, 32, 64, 41, (0, 13), (17, -29)),
    (10, 27, 20, 42, (6, 27), (11, 7)),
    (12, 37, 40, 43, (24,), (-26, 12)))


def pattern_search_golden(ref, cases=None, name="ref_pattern_search.npz"):
    """Config 4: what the reference's OWN TEncSearch::xPatternSearch (TEncSearch.cpp:3786-3848: SAD + vector cost, raster order, strict <)
    returns for every in-picture CU node of whole CTUs -- vector, SAD, cost -- on the seeded pan clip (original planes, zero predictor).
    The planes are stored with the expected outputs (data only)."""
    import ctypes as C
    oracle = op.load_oracle()
    ref.href_pattern_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    W, H = 416, 240
    cases = PATTERN_SEARCH_CASES if cases is None else cases
    out = {"cases": np.array([list(c[:4]) for c in cases], np.int32)}
    total = 0
    for k, case in enumerate(cases):
        (bd, qp, rng, seed, ctus), speeds = case[:5], (case[5] if len(case) > 5 else (3, 3))
        ys = frames.pan_clip(W, H, 2, seed=seed, v_structure=speeds[0], v_noise=speeds[1])
        (rb, org, stride), (cb, _, _) = [frames.to_pel_plane(y, bd) for y in ys]
        if bd > 8:  # use the low bits too
            cb = (cb + np.random.default_rng(bd).integers(0, 1 << (bd - 8), size=cb.shape, dtype=np.int16)).astype(np.int16)
            rb = (rb + np.random.default_rng(bd + 1).integers(0, 1 << (bd - 8), size=rb.shape, dtype=np.int16)).astype(np.int16)
        cur = np.ascontiguousarray(cb.reshape(-1)[org:].copy()[: (H - 1) * stride + W])  # from sample (0, 0) on, HM stride
        refp = np.ascontiguousarray(rb.reshape(-1)[org:].copy()[: (H - 1) * stride + W])
        lam = oracle.fho_lambda_intra(qp, bd)
        res = np.full((len(ctus), 85, 4), -1, np.int32)
        for ci, c in enumerate(ctus):
            cx, cy = c % 7, c // 7
            blocks, where = [], []
            idx = 0
            for lvl in range(4):
                n, cnt = 64 >> lvl, 1 << lvl
                for by in range(cnt):
                    for bx in range(cnt):
                        x0, y0 = cx * 64 + bx * n, cy * 64 + by * n
                        if x0 + n <= W and y0 + n <= H:
                            blocks.append((x0, y0, n)); where.append(idx)
                        idx += 1
            b = np.array(blocks, np.int32)
            o = np.zeros((len(blocks), 4), np.int32)
            assert ref.href_pattern_search(cur.ctypes.data, refp.ctypes.data, stride, W, H, bd, C.c_double(lam), rng, len(blocks), b.ctypes.data, o.ctypes.data) == len(blocks)
            res[ci, where] = o
            total += len(blocks)
        out[f"cur{k}"], out[f"ref{k}"], out[f"stride{k}"] = cur, refp, np.int32(stride)
        out[f"ctus{k}"], out[f"nodes{k}"] = np.array(ctus, np.int32), res
    dst = os.path.join(os.path.dirname(HERE), "tests", "golden", name)
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", total, "nodes searched by the reference's xPatternSearch")


def _pattern_nodes(ref, cur, refp, stride, W, H, bd, lam, rng, ctus):
    """xPatternSearch on every in-picture CU node of the given CTUs -> [len(ctus), 85, 4] (mvx, mvy, SAD, cost; -1 outside)."""
    import ctypes as C
    cw = (W + 63) // 64
    res = np.full((len(ctus), 85, 4), -1, np.int32)
    for ci, c in enumerate(ctus):
        cx, cy = c % cw, c // cw
        blocks, where = [], []
        idx = 0
        for lvl in range(4):
            n, cnt = 64 >> lvl, 1 << lvl
            for by in range(cnt):
                for bx in range(cnt):
                    x0, y0 = cx * 64 + bx * n, cy * 64 + by * n
                    if x0 + n <= W and y0 + n <= H:
                        blocks.append((x0, y0, n)); where.append(idx)
                    idx += 1
        b = np.array(blocks, np.int32)
        o = np.zeros((len(blocks), 4), np.int32)
        assert ref.href_pattern_search(cur.ctypes.data, refp.ctypes.data, stride, W, H, bd, C.c_double(lam), rng, len(blocks),
                                       b.ctypes.data, o.ctypes.data) == len(blocks)
        res[ci, where] = o
    return res


def bit_depths_golden(ref):
    """tests/golden/ref_bit_depths.npz: the reference's own SATD (calcHAD / xGetHADs), reference-sample fill, 35 predictors,
    initIntraPatternChType lines, pre-analysis / xComputeQP and xPatternSearch at bit depths 9 to 12 and on full-swing samples
    (0 against 2^bd - 1).  The inputs are regenerated from seeds (oracle/bd_cases.py); the file holds case lists and outputs.

    HM was built with RExt__HIGH_BIT_DEPTH_SUPPORT 0 (Pel = 16 bit); every function here accepted every depth 9 to 12."""
    import ctypes as C
    from oracle import bd_cases as bc
    oracle = op.load_oracle()
    out = {"hm_version": np.frombuffer(ref.href_version(), np.uint8)}

    meta, calc, get = [], [], []
    for bd in bc.SATD_BIT_DEPTHS:
        for (w, h) in bc.SATD_SHAPES:
            for rep, kind in enumerate(bc.SATD_KINDS):
                a, b = bc.satd_pair(bd, w, h, kind, rep)
                get.append(ref.href_get_hads(bd, op.ptr(a), 64, op.ptr(b), 64, w, h))
                calc.append(ref.href_calc_had(bd, op.ptr(a), 64, op.ptr(b), 64, w, h) if (w % 4 == 0 and h % 4 == 0) else 0xFFFFFFFF)
                meta.append((bd, w, h, rep))
    out["satd_meta"] = np.array(meta, np.int32)
    out["satd_calchad"], out["satd_gethads"] = np.array(calc, np.uint32), np.array(get, np.uint32)

    for bd in bc.INTRA_BIT_DEPTHS:
        for n in bc.INTRA_SIZES:
            lines = []
            for rep in range(bc.FILL_REPS):
                pic, flags = bc.fill_case(bd, n, rep)
                roi = np.zeros((2 * n + 1) * (2 * n + 1), np.int16)
                side = pic.shape[1]
                ref.href_fill_ref(bd, op.ptr(pic.reshape(-1), 4 * side + 4), side, flags, n, roi)
                lines.append(op.roi_to_ref_line(roi.reshape(2 * n + 1, 2 * n + 1), n))
            out[f"fill_n{n}_bd{bd}"] = np.stack(lines)
            for kind in ("sat", "flat"):
                roi = np.ascontiguousarray(op.ref_line_to_roi(bc.pred_line(bd, n, kind), n).reshape(-1))
                preds = np.zeros((35, n, n), np.int16)
                for m in range(35):
                    p = np.zeros(n * n, np.int16)
                    ref.href_pred_intra(roi, n, m, bd, p)
                    preds[m] = p.reshape(n, n)
                out[f"pred_{kind}_n{n}_bd{bd}"] = preds

    lib = op.bind_rdo(ref)
    lib.href_intra_lines.argtypes = [C.c_int] * 7 + [C.c_void_p, C.c_void_p]
    for k, (content, w, h, bd, qp, ctus) in enumerate(bc.INTRA_LINE_CASES):
        buf, org, stride = bc.intra_line_plane(content, w, h, bd)
        op.rdo_encode(lib, buf, org, stride, w, h, bd, qp)
        cw = (w + 63) // 64
        meta, unf, flt = [], [], []
        first = True
        for c in ctus:
            for depth in range(4):
                n = 64 >> depth
                for by in range(1 << depth):
                    for bx in range(1 << depth):
                        x0, y0 = (c % cw) * 64 + bx * n, (c // cw) * 64 + by * n
                        if x0 + n > w or y0 + n > h:
                            continue
                        a, b = np.zeros(4 * n + 1, np.int16), np.zeros(4 * n + 1, np.int16)
                        rc = lib.href_intra_lines(w, h, bd, c, depth, (by * n // 4) * 16 + bx * n // 4, 1 if first else 0, a.ctypes.data, b.ctypes.data)
                        assert rc == 4 * n + 1, rc
                        first = False
                        meta.append((c, depth, x0, y0, n)); unf.append(a); flt.append(b)
        out[f"lines_meta{k}"], out[f"lines_unf{k}"], out[f"lines_flt{k}"] = np.array(meta, np.int32), np.concatenate(unf), np.concatenate(flt)

    for k, (content, w, h, bd, depth) in enumerate(bc.PREANALYZE_CASES):
        buf, org, stride = bc.preanalyze_plane(content, w, h, bd)
        n = sum(((w + (64 >> d) - 1) // (64 >> d)) * ((h + (64 >> d) - 1) // (64 >> d)) for d in range(depth))
        act, avg = np.zeros(n), np.zeros(depth)
        assert ref.href_preanalyze(op.ptr(buf.reshape(-1), org), stride, w, h, bd, depth, act, avg) == n
        out[f"pre_act{k}"], out[f"pre_avg{k}"] = act, avg
        for s, (range_, qp) in enumerate(bc.AQ_SETTINGS):
            q = np.zeros(n, np.int32)
            assert ref.href_aq_qp(op.ptr(buf.reshape(-1), org), stride, w, h, bd, depth, range_, qp, q) == n
            out[f"pre_qp{k}_{s}"] = q.astype(np.int8)

    ref.href_pattern_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    for k, (bd, qp, rng, content, seed, ctus) in enumerate(bc.PATTERN_CASES):
        cur, refp, stride = bc.pattern_planes(bd, content, seed)
        out[f"ps_nodes{k}"] = _pattern_nodes(ref, cur, refp, stride, 416, 240, bd, oracle.fho_lambda_intra(qp, bd), rng, ctus)

    dst = os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_bit_depths.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


# ---- config 4: the searches of the rectangular PUs and the quarter-sample stage (tests/golden/ref_pattern_search_pu.npz, ref_frac_search.npz) --------
# One ragged picture, 176 x 144 = 3 x 3 CTUs with a last column 48 wide and a last row 16 tall; whole CTUs: corner, ragged right, interior, ragged
# bottom, both.  Entries per CTU: the 85 nodes, the 124 PUs (motion_pu_ref.covered), the 384 small PUs (motion_pu_small_ref.covered).
PU_W, PU_H, PU_CTUS = 176, 144, (0, 2, 4, 6, 8)
PU_PAN_SPEEDS = ((2, -3), (-4, 6))   # (v_structure, v_noise) of the two pan clips
# (bit depth, QP, range, content): content 0 / 1 = the pan clip at that speed; every bit depth, QP and range with each of the others' values once
PU_PAN_CASES = ((8, 0, 1, 0), (8, 32, 5, 1), (8, 51, 8, 0), (10, 0, 5, 0), (10, 32, 8, 1), (10, 51, 1, 0), (12, 0, 8, 1), (12, 32, 1, 0), (12, 51, 5, 1))
# "white": the current picture 2^bd - 1 everywhere over a black reference (every vector has the same SAD); "checker": a one-sample checkerboard
# of 0 and 2^bd - 1 against its inverse (every vector with an odd x + y has SAD 0 away from the border: (0, -1) is the first of the cheapest in raster order)
PU_SEARCH_CASES = PU_PAN_CASES + ((10, 32, 5, "white"), (12, 0, 8, "checker"))
# "blend": the current picture is the reference blended with itself one sample away, direction and weight drawn per 8x8 cell (motion of about a half
# or a quarter sample: most winners are fractional); "flat": two different flat pictures (every candidate has the same distortion: the centre wins
# both stages); "swing": random samples of 0 and 2^bd - 1 (the filters overshoot both ends: the clip works)
PU_FRAC_CASES = PU_PAN_CASES + ((8, 27, 3, "blend"), (10, 22, 4, "blend"), (10, 32, 2, "flat"), (8, 12, 8, "swing"), (12, 37, 6, "swing"))


_PU_ENTRIES = []


def _pu_entries():
    """(rectangles (x0, y0, w, h), CU nodes (x0, y0, n)) of the 593 entries of one CTU in file order: 85 + 124 + 384, coordinates inside the CTU"""
    if _PU_ENTRIES:
        return _PU_ENTRIES
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import motion_pu_ref as mp
    import motion_pu_small_ref as ps
    rects = [mp.node_rect(k)[:2] + (mp.node_rect(k)[2],) * 2 for k in range(85)] + [mp.pu_rect(*e) for e in mp.covered()] + [mp.pu_rect(*e) for e in ps.covered()]
    nodes = list(range(85)) + [e[0] for e in mp.covered()] + [e[0] for e in ps.covered()]
    _PU_ENTRIES.extend((rects, [mp.node_rect(k) for k in nodes]))
    return _PU_ENTRIES


def _pu_planes(bd, content):
    """-> (cur, ref) int16 [H, W]"""
    hi = (1 << bd) - 1
    if content in (0, 1):
        ys = frames.pan_clip(PU_W, PU_H, 2, seed=70 + content, v_structure=PU_PAN_SPEEDS[content][0], v_noise=PU_PAN_SPEEDS[content][1])
        ref, cur = (y.astype(np.int64) << (bd - 8) for y in ys)
        if bd > 8:  # use the low bits too
            cur = cur + np.random.default_rng(bd).integers(0, 1 << (bd - 8), size=cur.shape)
            ref = ref + np.random.default_rng(bd + 1).integers(0, 1 << (bd - 8), size=ref.shape)
    elif content == "white":
        cur, ref = np.full((PU_H, PU_W), hi), np.zeros((PU_H, PU_W), np.int64)
    elif content == "checker":
        yy, xx = np.mgrid[0:PU_H, 0:PU_W]
        ref = ((yy + xx) % 2) * hi
        cur = hi - ref
    elif content == "flat":
        cur, ref = np.full((PU_H, PU_W), hi // 3), np.full((PU_H, PU_W), hi // 2)
    elif content == "swing":
        rng = np.random.default_rng(900 + bd)
        ref = rng.integers(0, 2, size=(PU_H, PU_W)) * hi
        cur = np.where(rng.random((PU_H, PU_W)) < 0.1, hi - ref, ref)
    else:  # "blend"
        rng = np.random.default_rng(800 + bd)
        ref = frames.pan_clip(PU_W, PU_H, 1, seed=72)[0].astype(np.int64) << (bd - 8)
        if bd > 8:
            ref = ref + rng.integers(0, 1 << (bd - 8), size=ref.shape)
        p = np.pad(ref, 1, mode="edge")
        cells = (PU_H // 8, PU_W // 8)
        dx, dy, wt = (rng.integers(lo, hi_, size=cells).repeat(8, 0).repeat(8, 1) for lo, hi_ in ((-1, 2), (-1, 2), (1, 3)))
        yy, xx = np.mgrid[0:PU_H, 0:PU_W]
        far = p[yy + 1 + dy, xx + 1 + dx]
        cur = np.where(wt == 2, (ref + far + 1) >> 1, (3 * ref + far + 2) >> 2)
    return np.ascontiguousarray(cur, np.int16), np.ascontiguousarray(ref, np.int16)


def _pu_blocks(c):
    """the entries of CTU c whose CU node lies wholly inside the picture -> (indices into the 593, [n, 4] picture rectangles)"""
    rects, nodes = _pu_entries()
    cx, cy = c % 3, c // 3
    where = [i for i, (nx, ny, n) in enumerate(nodes) if 64 * cx + nx + n <= PU_W and 64 * cy + ny + n <= PU_H]
    return where, np.array([(64 * cx + rects[i][0], 64 * cy + rects[i][1], rects[i][2], rects[i][3]) for i in where], np.int32)


def _pu_search_case(ref, oracle, cur, refp, bd, qp, R):
    """xPatternSearch on every valid entry of the five CTUs -> [5, 593, 5] int32: mvx, mvy, SAD, cost, SAD at the zero vector; -1 = outside"""
    import ctypes as C
    lam = C.c_double(oracle.fho_lambda_intra(qp, bd))
    res = np.full((len(PU_CTUS), 593, 5), -1, np.int32)
    for ci, c in enumerate(PU_CTUS):
        where, blocks = _pu_blocks(c)
        o, z = np.zeros((len(where), 4), np.int32), np.zeros((len(where), 4), np.int32)
        for rng, dst in ((R, o), (0, z)):
            assert ref.href_pattern_search_rect(cur.ctypes.data, refp.ctypes.data, PU_W, PU_W, PU_H, bd, lam, rng, len(where), blocks.reshape(-1), dst.reshape(-1)) == len(where)
        assert not z[:, :2].any()
        res[ci, where, :4], res[ci, where, 4] = o, z[:, 2]
    return res


def _pu_family_counts(valid):
    """valid [.., 593] -> valid entries per family: nodes, PUs, small PUs"""
    return [int(valid[..., :85].sum()), int(valid[..., 85:209].sum()), int(valid[..., 209:].sum())]


def _pu_save(name, out):
    dst = os.path.join(os.path.dirname(HERE), "tests", "golden", name)
    np.savez_compressed(dst, **out)
    size = os.path.getsize(dst)
    assert size < 1044550, (name, size)   # below the largest committed golden (ref_vectors.npz)
    print("wrote", dst, size, "bytes")


def motion_pu_golden(ref):
    """What the reference's OWN xPatternSearch (SAD, on w x h patterns) and xPatternSearchFracDIF (Hadamard, quarter-sample stage fed the integer
    search's vectors: HM's chain) return for every node and PU of five CTUs of a ragged picture.  Planes and integers only."""
    import ctypes as C
    oracle = op.load_oracle()
    planes, plane_of = [], {}

    def plane_index(bd, content):
        if (bd, content) not in plane_of:
            plane_of[(bd, content)] = len(planes)
            planes.append(_pu_planes(bd, content))
        return plane_of[(bd, content)]

    # ---- integer search
    out = {"size": np.array([PU_W, PU_H], np.int32), "ctus": np.array(PU_CTUS, np.int32)}
    cases, counts = [], np.zeros(3, np.int64)
    for k, (bd, qp, R, content) in enumerate(PU_SEARCH_CASES):
        p = plane_index(bd, content)
        res = _pu_search_case(ref, oracle, *planes[p], bd, qp, R)
        out[f"res{k}"] = res
        cases.append((bd, qp, R, p))
        counts += _pu_family_counts(res[..., 3] != -1)
    for p, (cur, refp) in enumerate(planes):
        out[f"cur{p}"], out[f"ref{p}"] = cur, refp
    out["cases"], out["counts"] = np.array(cases, np.int32), counts.astype(np.int32)
    print("integer search, valid entries (nodes, PUs, small PUs):", counts.tolist(), "in", len(cases), "cases")
    _pu_save("ref_pattern_search_pu.npz", out)

    # ---- fractional search around the integer search's own vectors; every 7th entry a seeded random vector instead, in the corner CTUs the
    # window's own corners: the replicated border is read
    planes, plane_of = [], {}
    out = {"size": np.array([PU_W, PU_H], np.int32), "ctus": np.array(PU_CTUS, np.int32)}
    cases, counts = [], np.zeros(3, np.int64)
    half_wins, quarter_wins = np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64)
    for k, (bd, qp, R, content) in enumerate(PU_FRAC_CASES):
        p = plane_index(bd, content)
        cur, refp = planes[p]
        ints = _pu_search_case(ref, oracle, cur, refp, bd, qp, R)
        rng = np.random.default_rng(1000 + k)
        vin = np.zeros((len(PU_CTUS), 593, 2), np.int16)
        res = np.full((len(PU_CTUS), 593, 5), -1, np.int32)
        for ci, c in enumerate(PU_CTUS):
            where, blocks = _pu_blocks(c)
            v = ints[ci, where, :2].copy()
            rnd = rng.integers(-R, R + 1, size=v.shape)
            if c == 0:
                rnd[:] = -R
            if c == 8:
                rnd[:] = R
            seventh = np.array(where) % 7 == 0
            v[seventh] = rnd[seventh]
            b = np.ascontiguousarray(np.concatenate([blocks, v], axis=1), np.int32)
            o = np.zeros((len(where), 7), np.int32)
            assert ref.href_frac_search(cur.ctypes.data, refp.ctypes.data, PU_W, PU_W, PU_H, bd, C.c_double(oracle.fho_lambda_intra(qp, bd)), len(where),
                                        b.reshape(-1), o.reshape(-1)) == len(where)
            vin[ci, where] = v
            res[ci, where] = o[:, [4, 3, 2, 0, 1]]    # satd_int, satd_best, cost_best, mvx, mvy: the library's record
            q = o[:, :2] - 4 * v - 2 * o[:, 5:7]
            np.add.at(half_wins, (o[:, 6] + 1, o[:, 5] + 1), 1)
            np.add.at(quarter_wins, (q[:, 1] + 1, q[:, 0] + 1), 1)
        out[f"in{k}"], out[f"out{k}"] = vin, res
        cases.append((bd, qp, R, p))
        counts += _pu_family_counts(res[..., 2] != -1)
    assert half_wins.all() and quarter_wins.all(), (half_wins, quarter_wins)   # every candidate of both tables wins somewhere
    for p, (cur, refp) in enumerate(planes):
        out[f"cur{p}"], out[f"ref{p}"] = cur, refp
    out["cases"], out["counts"] = np.array(cases, np.int32), counts.astype(np.int32)
    print("fractional search, valid entries (nodes, PUs, small PUs):", counts.tolist(), "in", len(cases), "cases")
    print("half-stage winners [dy + 1][dx + 1]:", half_wins.tolist(), "quarter-stage winners:", quarter_wins.tolist())
    _pu_save("ref_frac_search.npz", out)


if __name__ == "__main__":
    if "--motion-pu-only" in sys.argv:
        motion_pu_golden(op.load_ref())
    elif "--intra-lines-only" in sys.argv:
        intra_lines_golden(op.load_ref())
    elif "--preanalyze-only" in sys.argv:
        preanalyze_golden(op.load_ref())
    elif "--bit-depths-only" in sys.argv:
        bit_depths_golden(op.load_ref())
    else:
        main()
