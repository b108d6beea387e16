"""GPU suite (-m gpu): keep_tone_match_u8 (csrc/keep_tone.hip) alone, against its numpy restatement (tests/tone_match_ref.py) -- integers, so
EXACTLY.  The shapes are the smallest that reach every way the kernel can go wrong: one pixel; a radius larger than both sides (5 x 7,
R = 48: the clamp dominates); rows whose length is no multiple of 8, so the int16 intermediate moves element by element (33 x 65, 130 x 31,
64 x 515) and one that does (512 x 512: 16 bytes at a time); several tiles on both axes (pass 1: 256 pixels x 8 rows, pass 2: 64 columns x
32 rows) with the last one short; R = 120 near the image height; an odd radius (R = 3), whose window is padded to an even start."""
import numpy as np
import pytest
import torch

import footprint as FP
from tone_match_ref import tone_match_ref

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine.tone import ToneMatcher, tone_taps

pytestmark = pytest.mark.gpu

NAME = 'keep_tone_match_u8'
#         F    h    w  sigma    R
TABLE = [(1, 1, 1, 0.5, 2), (1, 5, 7, 16, 48), (2, 33, 65, 4, 12), (1, 64, 515, 16, 48), (3, 130, 31, 40, 120), (1, 512, 512, 16, 48),
         (3, 512, 512, 1, 3)]


def ctaps(sigma):
    import ctypes
    t = tone_taps(sigma)
    return (ctypes.c_int16 * len(t))(*t.tolist()), (len(t) - 1) // 2, t


def launch(src, rst, sigma, offset=0):
    """One call on device copies of uint8 [F,h,w,3] arrays -> the output on the host.  ``offset``: src, rst and out start that many bytes
    (the scratch twice as many) into larger buffers: no alignment is asked of them."""
    F, h, w, _ = src.shape
    n = src.size
    taps, R, _ = ctaps(sigma)

    def view(arr=None, dtype=torch.uint8, off=offset):
        raw = torch.zeros(n + off + 16, dtype=dtype, device='cuda')
        v = raw[off:off + n].view(F, h, w, 3)
        if arr is not None:
            v.copy_(torch.from_numpy(arr))
        return v
    s, r, o = view(src), view(rst), view()
    scratch = view(dtype=torch.int16)
    assert s.data_ptr() % 2 == offset % 2
    L.call(NAME, s, r, o, scratch, F, h, w, taps, R)
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy(), src) and np.array_equal(r.cpu().numpy(), rst)
    return o.cpu().numpy()


@pytest.mark.parametrize('case', TABLE, ids=lambda c: '%dx%dx%d-s%g' % c[:4])
def test_kernel_equals_the_restatement_exactly(case):
    F, h, w, sigma, R = case
    rng = np.random.default_rng(F * 1000003 + h * 1009 + w)
    src = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    rst = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    taps = tone_taps(sigma)
    assert len(taps) == 2 * R + 1
    want, clamped = tone_match_ref(src, rst, taps, with_clamped=True)
    if (h, w) == (33, 65):      # full-range noise: rst + delta leaves 0 .. 255 somewhere, so the final clamp is exercised
        assert clamped > 0 and not np.array_equal(want, rst)
    got = launch(src, rst, sigma)
    assert got.dtype == np.uint8 and np.array_equal(got, want), case
    assert np.array_equal(launch(src, rst, sigma, offset=1), want), (case, 'unaligned')


def test_the_extremes_reach_the_largest_intermediates():
    hi, lo = np.full((1, 64, 64, 3), 255, np.uint8), np.zeros((1, 64, 64, 3), np.uint8)
    taps = tone_taps(16)
    out, h4, v = tone_match_ref(hi, lo, taps, with_bounds=True)
    assert h4 == 4080 and v == 4080 * 4096 and (out == 255).all()
    assert (launch(hi, lo, 16) == 255).all() and (launch(lo, hi, 16) == 0).all()


@pytest.mark.parametrize('hw', [(5, 7), (33, 65), (128, 128)], ids=lambda s: '%dx%d' % s)
def test_identity_and_constant_shift_on_the_device(hw):
    h, w = hw
    rst = np.random.default_rng(h * w).integers(40, 200, (2, h, w, 3), dtype=np.uint8)
    assert np.array_equal(launch(rst, rst, 16), rst)
    for c in (-37, -1, 1, 40):
        src = (rst.astype(np.int64) + c).astype(np.uint8)
        assert np.array_equal(launch(src, rst, 16), src), c


def test_a_batch_equals_each_face_alone_and_two_runs_are_identical():
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (3, 70, 300, 3), dtype=np.uint8)
    rst = rng.integers(0, 256, (3, 70, 300, 3), dtype=np.uint8)
    whole = launch(src, rst, 4)
    assert np.array_equal(launch(src, rst, 4), whole)
    for i in range(3):
        assert np.array_equal(launch(src[i:i + 1], rst[i:i + 1], 4), whole[i:i + 1]), i
    assert np.array_equal(whole, tone_match_ref(src, rst, tone_taps(4)))


def test_33_faces_through_the_matcher_are_two_launches_and_equal_the_restatement(monkeypatch):
    rng = np.random.default_rng(33)
    src = rng.integers(0, 256, (33, 40, 24, 3), dtype=np.uint8)
    rst = rng.integers(0, 256, (33, 40, 24, 3), dtype=np.uint8)
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append((name, a[4])), real(name, *a))[1])
    tm = ToneMatcher('cuda')
    got = tm.match(src, torch.from_numpy(rst).cuda(), 2.0)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == src.shape
    assert calls == [(NAME, 32), (NAME, 1)]
    assert np.array_equal(got.cpu().numpy(), tone_match_ref(src, rst, tone_taps(2.0)))
    again = tm.match(src, rst, 2.0)
    assert again.data_ptr() != got.data_ptr() and torch.equal(again, got)
    assert len(tm._taps) == 1 and len(tm._scratch) == 1


@pytest.mark.parametrize('case', [(2, 33, 65, 4), (1, 40, 264, 16)], ids=lambda c: '%dx%dx%d-s%g' % c)
def test_footprint_in_poisoned_surroundings(case):
    """``out`` and ``scratch`` sit between guards; nothing outside them changes, the result does not depend on what surrounds ``src`` and
    ``rst``, and the two are unchanged (tests/footprint.py, as tests/test_gpu_footprint.py uses it).  33 x 65 takes the element-wise path of
    the intermediate, 40 x 264 (w % 8 == 0) the 16-byte one, with a second, short column tile in both passes."""
    F, h, w, sigma = case
    rng = np.random.default_rng(h)
    src = torch.from_numpy(rng.integers(0, 256, (F * h, w * 3), dtype=np.uint8))
    rst = torch.from_numpy(rng.integers(0, 256, (F * h, w * 3), dtype=np.uint8))
    taps, R, t = ctaps(sigma)
    regions = [FP.single('src', src), FP.single('rst', rst), FP.output('out', (F * h, w * 3), torch.uint8),
               FP.output('scratch', (F * h, w * 3), torch.int16, compare=False)]

    def run(T):
        assert all(T[k].is_contiguous() for k in T)
        L.call(NAME, T['src'], T['rst'], T['out'], T['scratch'], F, h, w, taps, R)
        torch.cuda.synchronize()
        assert torch.equal(T['src'].cpu(), src) and torch.equal(T['rst'].cpu(), rst)
    outs = FP.run(run, regions, 'cuda')
    want = tone_match_ref(src.numpy().reshape(F, h, w, 3), rst.numpy().reshape(F, h, w, 3), t)
    assert np.array_equal(outs['out'].cpu().numpy().reshape(F, h, w, 3), want)


def test_refused_calls_launch_nothing():
    taps, R, _ = ctaps(1)
    a, b = (torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device='cuda') for _ in range(2))
    out = torch.full((1, 4, 4, 3), 0xA5, dtype=torch.uint8, device='cuda')
    scratch = torch.zeros((1, 4, 4, 3), dtype=torch.int16, device='cuda')
    for args in ((a, b, out, scratch, 0, 4, 4, taps, R), (a, b, out, scratch, 1, 4, 32768, taps, R), (a, b, out, scratch, 1, 4, 4, taps, 0),
                 (a, b, b, scratch, 1, 4, 4, taps, R), (a, b, out, None, 1, 4, 4, taps, R)):
        with pytest.raises(L.KeepHipError, match=NAME) as e:
            L.call(NAME, *args)
        assert e.value.code == L.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
