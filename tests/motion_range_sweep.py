"""The expected records of the integer motion searches at EVERY search range from one pass, and the clips the sweep runs on
(tests/test_motion_range_sweep_ref.py pins this module without a GPU, tests/test_gpu_motion_range_sweep.py holds the kernels to it).

The SAD of a block at vector (dx, dy) in a border-replicated reference does not depend on the range, and neither does the vector cost: one
+-64 SAD volume per CTU (the 4x4 blocks of the CTU at every vector) gives every entry's distortion at every vector, and the winner at range R is
the first minimum of cost in raster order inside the sub-window of rows and columns 64 - R .. 64 + R.  The winners of all ranges come from one
pass over the volume: the key (cost, raster index) is minimised per ring of Chebyshev radius r, then accumulated over r -- the least key is the
raster-first vector of least cost, and the raster order of a sub-window is the raster order of the whole window restricted to it.  In SATD mode
(ranges 1..8 only, the MR = 8 kernels) the same is done on motion_pu_ref.tile_dists (8x8 Hadamards: nodes and the 124 PUs) and on
motion_pu_small_ref.quad_dists (4x4 Hadamards: the 384 small PUs) at +-8.

Geometry and entry order are motion_pu_ref's and motion_pu_small_ref's; an entry is valid iff its CU node lies wholly inside the picture.
Everything is cached at module scope per (clip, bit depth, QP, distortion).  A plain module, not a conftest and not a test."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import motion_pu_ref as mp
import motion_pu_small_ref as ps
import motion_refine_pu_ref as rp
import motion_refine_ref as mr
from fasthevc_amd import capi

DT, QDT = capi.MOTION_DTYPE, capi.MOTION_QPEL_DTYPE
MARKER = 0xFFFFFFFF
FAMS = ("nodes", "pu", "small")
PER = {"nodes": 85, "pu": mp.PUS_PER_CTU, "small": ps.PUS_SMALL_PER_CTU}
MAXR = 64


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------------

def entries(fam):
    """[(node, x0, y0, w, h)] of a family in output order, inside the CTU"""
    if fam == "nodes":
        return [(k,) + mp.node_rect(k) + (mp.node_rect(k)[2],) for k in range(85)]
    return [(k,) + mp.pu_rect(k, s, p) for k, s, p in (mp.covered() if fam == "pu" else ps.covered())]


ENTRIES = {f: entries(f) for f in FAMS}
assert [len(ENTRIES[f]) for f in FAMS] == [85, 124, 384]


def valid_entries(W, H):
    """{family: [numCtus, per CTU] bool}: the entry's CU node lies wholly inside the picture"""
    cw, ch = (W + 63) // 64, (H + 63) // 64
    out = {}
    for f in FAMS:
        v = np.zeros((cw * ch, PER[f]), bool)
        for c in range(cw * ch):
            w, h = min(64, W - 64 * (c % cw)), min(64, H - 64 * (c // cw))
            for i, (k, _, _, _, _) in enumerate(ENTRIES[f]):
                nx, ny, n = mp.node_rect(k)
                v[c, i] = nx + n <= w and ny + n <= h
        out[f] = v
    return out


# ---- distortions at every vector --------------------------------------------------------------------------------------------------------------------

def sad_volume(cur, ref, x0, y0, w, h, R=MAXR):
    """[h/4, w/4, 2R+1, 2R+1] (block row, block column, dy, dx): the SAD of every 4x4 block of region (x0, y0, w, h) of cur at every vector of
    [-R, R]^2 against ref with coordinates clamped to the picture; unshifted"""
    assert w % 4 == 0 and h % 4 == 0
    S = 2 * R + 1
    rpad = np.ascontiguousarray(mp.padded(ref, R).astype(np.int16))
    c = np.asarray(cur)[y0:y0 + h, x0:x0 + w].astype(np.int16)
    out = np.empty((h // 4, w // 4, S, S), np.int32)
    for dy in range(S):
        rows = rpad[y0 + dy:y0 + dy + h, x0:x0 + w + 2 * R]
        d = np.abs(sliding_window_view(rows, w, axis=1) - c[:, None, :])          # [h, S, w]: d[y, dx, x] = |cur[y, x] - ref[y + dy, x + dx]|
        d = d.view(np.uint16)                                                     # sixteen differences of at most 4095 fit 16 bits
        a = (d[:, :, 0::4] + d[:, :, 1::4] + d[:, :, 2::4] + d[:, :, 3::4]).reshape(h // 4, 4, S, w // 4)
        out[:, :, dy, :] = (a[:, 0] + a[:, 1] + a[:, 2] + a[:, 3]).transpose(0, 2, 1)
    return out


def integral(vol):
    """vol [bh, bw, S, S] -> [bh + 1, bw + 1, S, S]: the sums over the blocks above and to the left"""
    bh, bw, S, _ = vol.shape
    I = np.zeros((bh + 1, bw + 1, S, S), np.int32)
    I[1:, 1:] = vol.cumsum(axis=0, dtype=np.int32).cumsum(axis=1, dtype=np.int32)
    return I


def entry_sums(I, rects, shift):
    """I = integral(volume of 4x4 blocks), rects [(x0, y0, w, h)] in samples (multiples of 4, inside the volume) -> [len(rects), S, S]: the sum
    over each rectangle's blocks, shifted ONCE"""
    S = I.shape[2]
    out = np.empty((len(rects), S, S), np.int32)
    for i, (x0, y0, w, h) in enumerate(rects):
        a, b, c, d = x0 // 4, y0 // 4, (x0 + w) // 4, (y0 + h) // 4
        out[i] = (I[d, c] - I[b, c] - I[d, a] + I[b, a]) >> shift
    return out


def cost_window(oracle, R, sl):
    """[2R+1, 2R+1] (dy, dx) vector costs"""
    return mp.mv_costs(oracle, R, sl).reshape(2 * R + 1, 2 * R + 1)


def winners(E, costs):
    """E [n, S, S]: shifted distortions (dy, dx), costs [S, S], S = 2 Rmax + 1 -> [Rmax + 1, n] records: row R holds the winners of the sub-window
    64 - R .. 64 + R (row 0: the zero vector alone)"""
    n, S, _ = E.shape
    Rmax = S // 2
    dy, dx = np.mgrid[-Rmax:Rmax + 1, -Rmax:Rmax + 1]
    ring = np.maximum(np.abs(dy), np.abs(dx)).reshape(-1)
    order = np.argsort(ring, kind="stable")
    starts = np.searchsorted(ring[order], np.arange(Rmax + 1))
    flat = E.reshape(n, S * S)
    raster = np.arange(S * S, dtype=np.int64)
    assert S * S < (1 << 16)
    out = np.zeros((Rmax + 1, n), DT)
    for lo in range(0, n, 64):
        e = flat[lo:lo + 64].astype(np.int64)
        key = ((e + costs.reshape(-1)[None, :]) << 16) | raster[None, :]
        best = np.minimum.accumulate(np.minimum.reduceat(key[:, order], starts, axis=1), axis=1).T      # [Rmax + 1, m]
        idx = best & 0xFFFF
        o = out[:, lo:lo + 64]
        o["cost_best"] = best >> 16
        o["satd_best"] = np.take_along_axis(e, idx.T, axis=1).T
        o["satd_zero"] = e[:, (S * S - 1) // 2][None, :]
        o["mvx"], o["mvy"] = idx % S - Rmax, idx // S - Rmax
    return out


class PairSweep:
    """one picture pair: rec[family] = [Rmax + 1, numCtus, per CTU] records of every range (row 0 unused); markers where the CU node leaves the
    picture; CTUs not in `ctus` stay zero.  sad=False: the SATD mode of the MR = 8 kernels, Rmax = 8.  rmax: a smaller volume for pairs that
    are asked for small ranges only.  The distortions do not depend on the QP: at(qp) gives the records at another QP from the same volume as
    long as the sweep was created with more_qps naming it"""

    def __init__(self, oracle, cur, ref, bd, qp, sad=True, ctus=None, rmax=None, more_qps=()):
        cur, ref = np.asarray(cur, np.int64), np.asarray(ref, np.int64)
        H, W = cur.shape
        cw, ch = (W + 63) // 64, (H + 63) // 64
        self.W, self.H, self.bd, self.qp, self.sad = W, H, bd, qp, sad
        self.Rmax = rmax or (MAXR if sad else 8)
        assert sad or self.Rmax == 8
        self.ctus = list(range(cw * ch)) if ctus is None else list(ctus)
        self.valid = valid_entries(W, H)
        qps = [qp] + [q for q in more_qps if q != qp]
        costs = {q: cost_window(oracle, self.Rmax, mp.sqrt_lambda(oracle, q, bd)) for q in qps}
        self.by_qp = {q: {f: np.zeros((self.Rmax + 1, cw * ch, PER[f]), DT) for f in FAMS} for q in qps}
        for c in self.ctus:
            x0, y0 = 64 * (c % cw), 64 * (c // cw)
            E = self._sad(cur, ref, x0, y0) if sad else self._satd(cur, ref, x0, y0)
            for f in FAMS:
                ok = np.flatnonzero(self.valid[f][c])
                for q in qps:
                    r = self.by_qp[q][f][:, c]
                    r["satd_zero"], r["satd_best"], r["cost_best"] = MARKER, MARKER, MARKER
                    if len(ok):
                        r[:, ok] = winners(E[f], costs[q])
        for q in qps:
            for f in FAMS:
                self.by_qp[q][f][0] = 0
        self.rec = self.by_qp[qp]

    def at(self, qp, R):
        """{family: [numCtus, per CTU]} at range R and one of the sweep's QPs"""
        assert 1 <= R <= self.Rmax
        return {f: self.by_qp[qp][f][R] for f in FAMS}

    def _sad(self, cur, ref, x0, y0):
        w, h = min(64, self.W - x0) // 4 * 4, min(64, self.H - y0) // 4 * 4       # blocks not wholly inside the picture contribute nothing
        vol = integral(sad_volume(cur, ref, x0, y0, w, h, self.Rmax))
        c = (y0 // 64) * ((self.W + 63) // 64) + x0 // 64
        return {f: entry_sums(vol, [e[1:] for e, v in zip(ENTRIES[f], self.valid[f][c]) if v], self.bd - 8) for f in FAMS}

    def _satd(self, cur, ref, x0, y0):
        w, h = min(64, self.W - x0), min(64, self.H - y0)
        c = (y0 // 64) * ((self.W + 63) // 64) + x0 // 64
        td = mp.tile_dists(cur, ref, 8, False, x0, y0, w // 8 * 8, h // 8 * 8)
        qd = ps.quad_dists(cur, ref, 8, False, x0, y0, w // 4 * 4, h // 4 * 4)
        out = {}
        for f in FAMS:
            rects = [e[1:] for e, v in zip(ENTRIES[f], self.valid[f][c]) if v]
            if f == "small":
                s = [ps.quad_sum(qd, self.bd, *r) for r in rects]
            else:
                s = [td[:, r[1] // 8:(r[1] + r[3]) // 8, r[0] // 8:(r[0] + r[2]) // 8].sum(axis=(1, 2)) >> (self.bd - 8) for r in rects]
            out[f] = np.array(s, np.int32).reshape(len(rects), 17, 17)
        return out

    def records(self, R):
        """{family: [numCtus, per CTU]} at range R"""
        return self.at(self.qp, R)


# ---- the sweep clips ----------------------------------------------------------------------------------------------------------------------------------

W, H, NF = 104, 88, 3      # a 2 x 2 CTU grid: one whole CTU, one 40 wide, one 24 tall, the corner; every window reaches a replicated border at every range
CLIPS = ("diag", "anti", "slow")
# clip -> (ramp direction (sx, sy), position of the smooth layer per picture in samples along that direction, fade per picture in levels,
#          motion of the moving texture per picture, seed, QP the sweep runs it at per bit depth)
_CLIP = {
    "diag": ((1, 1), (0, 96, 0), (0, 0, 0), (0, 0), 11, {8: 14, 10: 19, 12: 23}),
    "anti": ((1, -1), (0, -96, 0), (0, 0, 0), (0, 0), 12, {8: 17, 10: 13, 12: 20}),
    "slow": ((1, 1), (0, 13, 26), (0, 90, 0), (13, -9), 13, {8: 22, 10: 24, 12: 16}),
}
_PICS, _SWEEPS = {}, {}


def clip(name):
    """three uint8 pictures [H, W].  Smooth plus texture: the smooth layer is a ramp of half a level per sample along one diagonal with two
    shallow waves on it; the texture is binary noise at full swing (0 / 255: a smooth block is never nearer to it than to the ramp, so it attracts
    none) in 8x8 cells of the picture's central cross (the four corner regions stay smooth), some cells static, the others moving.
      diag: the smooth layer pans by 96 samples along (+1, +1) and back -- further than any window reaches, so a block's best match lies at the
            window's corner: (-R, -R) in the first pair, (+R, +R) in the second; the texture cells stand still and win at the zero vector
      anti: the same along (+1, -1) in the opposite sense: corners (+R, -R), then (-R, +R)
      slow: the smooth layer pans by 13 samples per picture and the moving texture by (13, -9), inside +-20; a fade of 90 levels up and down
            again sends the smooth blocks to the corners as in diag, the moving texture wins inside the window from R = 13 on
    The ramp keeps rising across the whole picture, so even at R = 64 the SAD of a block that is brighter (darker) than the whole reference still
    falls over the last step towards the corner as long as one of its columns and rows is inside the picture there."""
    if name not in _PICS:
        (sx, sy), pos, fade, tv, seed, _ = _CLIP[name]
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        cells = rng.integers(0, 3, size=(H // 8, W // 8)).repeat(8, 0).repeat(8, 1)          # 0 smooth, 1 static texture, 2 moving texture
        cells[(np.abs(xx - 52) >= 12) & (np.abs(yy - 44) >= 20)] = 0                       # the central cross only
        noise = 255.0 * rng.integers(0, 2, size=(H, W))                                     # full swing: no smooth block is nearer to it than to the ramp
        level = [fade[t] - pos[t] for t in range(NF)]          # the smooth layer's brightness per picture: half a level per sample, two axes
        base = 128 - (max(level) + min(level)) / 2.0
        pics = []
        for t in range(NF):
            u = sx * (xx - pos[t] * sx) + sy * (yy - pos[t] * sy)
            smooth = base + 0.5 * (u - (sx * 52 + sy * 44)) + 3.0 * np.sin((xx - pos[t] * sx) / 13.0) + 3.0 * np.cos((yy - pos[t] * sy) / 11.0) + fade[t]
            moved = np.roll(np.roll(noise, tv[0] * t, axis=1), tv[1] * t, axis=0)
            mcell = np.roll(np.roll(cells == 2, tv[0] * t, axis=1), tv[1] * t, axis=0)
            y = np.where(cells == 1, noise, smooth)
            y = np.where(mcell & (cells != 1), moved, y)
            pics.append(np.clip(np.rint(y), 0, 255).astype(np.uint8))
        _PICS[name] = pics
    return _PICS[name]


def clip_qp(name, bd):
    return _CLIP[name][5][bd]


def planes(name, bd):
    """the clip at bd bits: [H, W] int64 per picture, the low bits populated above 8 bit (motion_gpu_helpers.clip_planes)"""
    from motion_gpu_helpers import clip_planes
    return clip_planes(clip(name), bd, low_bits_seed=_CLIP[name][4])


def sweep(oracle, name, bd, sad=True):
    """[PairSweep of pictures (0, 1), PairSweep of pictures (1, 2)] of a clip at its QP; computed once"""
    key = (name, bd, clip_qp(name, bd), sad)
    if key not in _SWEEPS:
        p = planes(name, bd)
        _SWEEPS[key] = [PairSweep(oracle, p[f + 1], p[f], bd, key[2], sad=sad) for f in range(NF - 1)]
    return _SWEEPS[key]


def expected(oracle, name, bd, R, sad=True):
    """{family: [NF - 1, numCtus, per CTU]}: what a device call over the clip's three pictures must write at range R"""
    s = sweep(oracle, name, bd, sad)
    return {f: np.stack([p.rec[f][R] for p in s]) for f in FAMS}


def valid_counts(Wp=W, Hp=H):
    """{family: valid entries of one picture pair}, from the geometry alone"""
    return {f: int(v.sum()) for f, v in valid_entries(Wp, Hp).items()}


# ---- the refinements: memoised per (pair, CTU, family, entry, input vector) ------------------------------------------------------------------------------

class RefineMemo:
    """the quarter-sample refinement of a clip's entries (motion_refine_ref.refine_node for the nodes, motion_refine_pu_ref.refine_block for the PUs)
    around any input vectors.  A refinement depends on (pair, CTU, entry, input vector) only once the clip, the bit depth and the QP are fixed;
    the validity rule -- |mv| <= max_range, node inside -- is applied per call"""

    def __init__(self, oracle, name, bd):
        self.oracle, self.bd = oracle, bd
        p = planes(name, bd)
        self.sl = mr.sqrt_lambda(oracle, clip_qp(name, bd), bd)
        self.planes = [mr.Planes(p[f], bd, MAXR + 8) for f in range(NF - 1)]
        self.cur = [np.ascontiguousarray(p[f + 1].astype(np.int16)).reshape(-1) for f in range(NF - 1)]
        self.valid = valid_entries(W, H)
        self.memo = {}
        self.computed = 0

    def one(self, pair, c, f, i, mx, my):
        key = (pair, c, f, i, mx, my)
        if key not in self.memo:
            _, x0, y0, w, h = ENTRIES[f][i]
            x0, y0 = x0 + 64 * (c % 2), y0 + 64 * (c // 2)
            if f == "nodes":
                r = mr.refine_node(self.oracle, self.planes[pair], self.cur[pair], 0, W, x0, y0, w, mx, my, self.sl)
            else:
                r = rp.refine_block(self.oracle, self.planes[pair], self.cur[pair], 0, W, x0, y0, w, h, mx, my, self.sl)
            self.memo[key] = (r["satd_int"], r["satd_best"], r["cost_best"], r["mvx"], r["mvy"])
            self.computed += 1
        return self.memo[key]

    def expected(self, ins, max_range):
        """ins: {family: [NF - 1, numCtus, per CTU]} with mvx / mvy -> the same shapes of MOTION_QPEL_DTYPE"""
        out = {}
        for f, a in ins.items():
            o = np.zeros(a.shape, QDT)
            for pair in range(a.shape[0]):
                for c in range(a.shape[1]):
                    for i in range(a.shape[2]):
                        mx, my = int(a["mvx"][pair, c, i]), int(a["mvy"][pair, c, i])
                        if not self.valid[f][c, i] or abs(mx) > max_range or abs(my) > max_range:
                            o[pair, c, i] = (MARKER, MARKER, MARKER, 0, 0)
                        else:
                            o[pair, c, i] = self.one(pair, c, f, i, mx, my)
            out[f] = o
        return out


_MEMOS = {}


def refine_memo(oracle, name, bd):
    if (name, bd) not in _MEMOS:
        _MEMOS[(name, bd)] = RefineMemo(oracle, name, bd)
    return _MEMOS[(name, bd)]
