"""The two goldens of the PU motion searches and of the quarter-sample stage as the tests read them (test_oracle_golden_motion_pu.py without a GPU,
test_gpu_motion_golden.py on one): tests/golden/ref_pattern_search_pu.npz holds what the reference's own xPatternSearch returned (SAD, w x h
patterns), tests/golden/ref_frac_search.npz what its xPatternSearchFracDIF returned around given integer vectors, for the 85 nodes, the 124 PUs
(motion_pu_ref.covered) and the 384 small PUs (motion_pu_small_ref.covered) of five whole CTUs of a ragged 176 x 144 picture
(oracle/gen_golden.py --motion-pu-only).  Nothing here computes an expected value: the files' integers are laid out as the library's records, with
the library's marker where the file holds -1 (the entry's CU node crosses the picture's edge).  A plain module, not a conftest."""
import os

import numpy as np

from fasthevc_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARKER = 0xFFFFFFFF
FAMILIES = {"nodes": slice(0, 85), "pu": slice(85, 209), "small": slice(209, 593)}   # the 593 entries of a CTU in the files' order
# valid entries per family in each file, as the generator printed them: every test asserts that it compared this many
SEARCH_COUNTS = {"nodes": 2937, "pu": 3828, "small": 13464}
FRAC_COUNTS = {"nodes": 3738, "pu": 4872, "small": 17136}


class Case:
    """one case of a file: bit depth, QP, range, the two pictures [H, W] (int16) and the file's integer arrays"""

    def __init__(self, z, k):
        self.k = k
        self.bd, self.qp, self.R, p = (int(v) for v in z["cases"][k])
        self.cur, self.ref = z[f"cur{p}"], z[f"ref{p}"]
        self.W, self.H = (int(v) for v in z["size"])
        self.ctus = [int(c) for c in z["ctus"]]
        self.num_ctus = ((self.W + 63) // 64) * ((self.H + 63) // 64)
        assert self.cur.shape == (self.H, self.W) and self.cur.dtype == np.int16 and self.ref.shape == self.cur.shape

    def __repr__(self):
        return f"case{self.k}(bd={self.bd}, qp={self.qp}, R={self.R})"


class SearchCase(Case):
    def __init__(self, z, k):
        super().__init__(z, k)
        self.res = z[f"res{k}"]       # [5, 593, 5]: mvx, mvy, SAD, cost, SAD at the zero vector

    def records(self, family):
        """[5, entries of the family] MOTION_DTYPE: what the library must write for the file's CTUs"""
        r = self.res[:, FAMILIES[family]].astype(np.int64)
        valid = r[..., 3] != -1
        out = np.zeros(valid.shape, capi.MOTION_DTYPE)
        for name, col in (("satd_zero", 4), ("satd_best", 2), ("cost_best", 3)):
            out[name] = np.where(valid, r[..., col], MARKER)
        out["mvx"], out["mvy"] = np.where(valid, r[..., 0], 0), np.where(valid, r[..., 1], 0)
        assert (r[~valid] == -1).all() and (r[valid][:, 2:] >= 0).all()
        return out


class FracCase(Case):
    def __init__(self, z, k):
        super().__init__(z, k)
        self.vin, self.out = z[f"in{k}"], z[f"out{k}"]   # [5, 593, 2] integer vectors; [5, 593, 5]: satd_int, satd_best, cost_best, mvx, mvy (quarter samples)

    def inputs(self, family, seed=0):
        """[numCtus, entries of the family] MOTION_DTYPE: the file's integer vectors in its CTUs (zero elsewhere) among random bytes -- only mvx
        and mvy may matter"""
        n = FAMILIES[family].stop - FAMILIES[family].start
        a = np.random.default_rng(seed).integers(0, 256, size=(self.num_ctus, n, 16), dtype=np.uint8).view(capi.MOTION_DTYPE).reshape(self.num_ctus, n)
        a["mvx"], a["mvy"] = 0, 0
        a["mvx"][self.ctus], a["mvy"][self.ctus] = self.vin[:, FAMILIES[family], 0], self.vin[:, FAMILIES[family], 1]
        return a

    def records(self, family):
        """[5, entries of the family] MOTION_QPEL_DTYPE"""
        r = self.out[:, FAMILIES[family]].astype(np.int64)
        valid = r[..., 2] != -1
        out = np.zeros(valid.shape, capi.MOTION_QPEL_DTYPE)
        for name, col in (("satd_int", 0), ("satd_best", 1), ("cost_best", 2)):
            out[name] = np.where(valid, r[..., col], MARKER)
        out["mvx"], out["mvy"] = np.where(valid, r[..., 3], 0), np.where(valid, r[..., 4], 0)
        assert (r[~valid] == -1).all() and (r[valid][:, :3] >= 0).all()
        return out


def _cases(name, cls, counts):
    z = np.load(os.path.join(GOLDEN, name))
    assert dict(zip(FAMILIES, (int(v) for v in z["counts"]))) == counts
    return [cls(z, k) for k in range(len(z["cases"]))]


def search_cases():
    return _cases("ref_pattern_search_pu.npz", SearchCase, SEARCH_COUNTS)


def frac_cases():
    return _cases("ref_frac_search.npz", FracCase, FRAC_COUNTS)


def same(got, exp, what=""):
    """every field of every entry, markers included (got / exp: [5, n] records of one dtype) -> the number of valid entries compared"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    for f in exp.dtype.names:
        bad = got[f] != exp[f]
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[f][bad][:5].tolist(), exp[f][bad][:5].tolist())
    return int((exp["cost_best"] != MARKER).sum())
