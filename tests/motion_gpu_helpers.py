"""What the GPU tests of the PU motion searches and of their quarter-sample refinement share (test_gpu_motion_pu.py, test_gpu_motion_pu_small.py,
test_gpu_motion_refine_pu.py): the device fixture, guarded device outputs, and pictures in TComPicYuv's layout.  A plain module, not a conftest."""
import numpy as np
import pytest

from fasthevc_amd import capi, frames

CANARY = 0xA5
DT = capi.MOTION_DTYPE


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


class Guarded:
    """nbytes of device output between two canary-filled guards of 4 KiB, everything pre-filled with the canary"""
    GUARD = 4096

    def __init__(self, torch, nbytes):
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * self.GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + self.GUARD

    def result(self, shape):
        h = self.t.cpu().numpy()
        assert (h[:self.GUARD] == CANARY).all() and (h[self.GUARD + self.n:] == CANARY).all(), "a guard around the output was written"
        return h[self.GUARD:self.GUARD + self.n].copy().view(DT).reshape(shape)

    def untouched(self):
        return bool((self.t.cpu().numpy() == CANARY).all())


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def same(got, exp, what=""):
    for k in DT.names:
        assert np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:5], got[k][got[k] != exp[k]][:5], exp[k][got[k] != exp[k]][:5])


def clip_planes(ys, bd, low_bits_seed=0):
    """uint8 pictures -> [H, W] int64 samples at bd bits per picture, with the low bits populated above 8 bit"""
    pics = []
    for i, y in enumerate(ys):
        p = y.astype(np.int64) << (bd - 8)
        if bd > 8:
            p = p + np.random.default_rng(low_bits_seed + i).integers(0, 1 << (bd - 8), size=p.shape)
        pics.append(p)
    return pics


def pel(pic):
    """[H, W] samples -> (buffer, origin, stride) in TComPicYuv's layout (zero margins)"""
    h, w = pic.shape
    m = frames.HM_MARGIN
    buf = np.zeros((h + 2 * m, w + 2 * m), np.int16)
    buf[m:m + h, m:m + w] = pic
    return buf, m * (w + 2 * m) + m, w + 2 * m


def pel_batch(pics):
    planes = [pel(p) for p in pics]
    return np.stack([p[0] for p in planes]), planes[0][1], planes[0][2], planes[0][0].size
