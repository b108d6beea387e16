"""GPU suite (-m gpu): keep_resize_linear_fxy_u8 (csrc/keep_resize_linear.hip, through engine/resize.py:LinearResizer.enlarge_u8) bit for
bit against the independent numpy restatement of ``cv2.resize(src, (0, 0), fx=f, fy=f, INTER_LINEAR)`` (tests/cv_linear_fxy_ref.py) at
``f = 512.0 / min(h, w)`` -- ``read_image``'s enlargement -- and the ``dsize`` entry, which shares its kernel, unchanged against its own
restatement (tests/cv_linear_ref.py)."""
import math

import numpy as np
import pytest
import torch

import cv_linear_fxy_ref as F
import cv_linear_ref as R

pytestmark = pytest.mark.gpu

# (h, w): landscape and portrait video, a 4.3 : 2 enlargement, one pixel short of no enlargement, a one-pixel axis
GEOMETRIES = [(360, 480), (480, 270), (240, 320), (511, 600), (1, 7)]
# the cases of tests/test_gpu_resize_linear.py
DSIZE = [((23, 31), (64, 64)), ((90, 120), (64, 64)), ((128, 96), (64, 48)), ((130, 96), (64, 48)), ((600, 800), (64, 64)),
         ((1, 9), (4, 20)), ((9, 1), (20, 4)), ((5, 7), (1, 1)), ((256, 256), (512, 512))]


@pytest.fixture(scope='module')
def rz():
    from comfyui_keep_amd.engine.resize import LinearResizer
    return LinearResizer('cuda')


def factor(h, w):
    return 512.0 / min(h, w)


_REF = {}


def reference(hw):
    """(frames [3,h,w,3], restatement [3,H2,W2,3]) of a geometry: computed once, shared, never written to."""
    if hw not in _REF:
        h, w = hw
        x = np.random.default_rng(h * 1000 + w).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
        ref = np.stack([F.resize_linear_fxy(fr, factor(h, w), factor(h, w)) for fr in x])
        x.setflags(write=False)
        ref.setflags(write=False)
        _REF[hw] = (x, ref)
    return _REF[hw]


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', GEOMETRIES)
def test_random_frames_equal_the_restatement(rz, hw, n):
    x, ref = reference(hw)
    f = factor(*hw)
    got = rz.enlarge_u8(torch.from_numpy(x[:n].copy()), f, f)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == ref[:n].shape
    got = got.cpu().numpy()
    print(f"{hw} x {f!r} -> {ref.shape[1:3]}, N = {n}: {int((got != ref[:n]).sum())} of {ref[:n].size} values differ from the restatement")
    assert np.array_equal(got, ref[:n]), np.argwhere(got != ref[:n])[:4]
    if n == 1:                                                           # an unbatched frame is the same launch
        one = rz.enlarge_u8(x[0].copy(), f, f)
        assert tuple(one.shape) == ref.shape[1:] and np.array_equal(one.cpu().numpy(), ref[0])


@pytest.mark.parametrize('hw', GEOMETRIES)
def test_the_extremes_stay_where_they_are(rz, hw):
    f = factor(*hw)
    w2, h2 = F.enlarged_size(hw[0], hw[1], f, f)
    for value in (0, 255):
        got = rz.enlarge_u8(np.full(hw + (3,), value, np.uint8), f, f)
        assert tuple(got.shape) == (h2, w2, 3) and bool((got == value).all()), value
    # a checkerboard of the two: every weight pair meets 0 and 255
    board = (np.indices(hw).sum(0) % 2 * 255).astype(np.uint8)[:, :, None].repeat(3, 2)
    assert np.array_equal(rz.enlarge_u8(board, f, f).cpu().numpy(), F.resize_linear_fxy(board, f, f))


def test_one_launch_into_a_slice_of_a_larger_batch(rz, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    x, ref = reference((240, 320))
    f = factor(240, 320)
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    into = torch.full((5,) + ref.shape[1:], 7, dtype=torch.uint8, device='cuda')
    assert rz.enlarge_u8(x.copy(), f, f, out=into[1:4]).data_ptr() == into[1].data_ptr()
    assert calls == ['keep_resize_linear_fxy_u8']
    assert np.array_equal(into[1:4].cpu().numpy(), ref) and bool((into[0] == 7).all()) and bool((into[4] == 7).all())
    with pytest.raises(ValueError):
        rz.enlarge_u8(x.copy(), f, f, out=into[1:3])


def test_the_rounded_size_is_not_the_scale(rz):
    """The case the entry exists for: at 360 x 480 the dsize entry, asked for the same 512 x 683, gives other pixels."""
    x, ref = reference((360, 480))
    assert not torch.equal(rz.resize_u8(x[0].copy(), 683, 512), rz.enlarge_u8(x[0].copy(), factor(360, 480), factor(360, 480)))


def test_refusals_launch_nothing(rz, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    lib = L.load()
    x = torch.zeros((1, 360, 480, 3), dtype=torch.uint8, device='cuda')
    y = torch.full((1, 512, 683, 3), 7, dtype=torch.uint8, device='cuda')
    f = factor(360, 480)
    with pytest.raises(L.KeepHipError, match='keep_resize_linear_fxy_u8'):
        L.call('keep_resize_linear_fxy_u8', x, y, 0, 360, 480, 512, 683, f, f)               # N = 0
    args = [x.data_ptr(), y.data_ptr(), 1, 360, 480, 512, 683, f, f, None]
    for i, bad in ((0, None), (1, None), (2, -1), (2, 70000), (3, 0), (4, -2), (5, 0), (6, 0), (5, 511), (6, 682), (6, 684),
                   (7, 0.0), (8, -f), (7, math.nan), (8, math.inf), (7, 1.0 / (683.0 / 480.0))):
        a = list(args)
        a[i] = bad
        assert lib.keep_resize_linear_fxy_u8(*a) == -1, (i, bad)
        assert lib.keep_last_error().startswith(b'keep_resize_linear_fxy_u8'), lib.keep_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7).all())                                                               # nothing ran
    monkeypatch.setattr(L, 'call', lambda *a: pytest.fail(f"launched {a[0]}"))
    empty = rz.enlarge_u8(torch.zeros((0, 360, 480, 3), dtype=torch.uint8), f, f)
    assert tuple(empty.shape) == (0, 512, 683, 3) and empty.is_cuda
    with pytest.raises(ValueError):
        rz.enlarge_u8(np.zeros((360, 480), np.uint8), f, f)


@pytest.mark.parametrize('hw,hw2', DSIZE)
def test_the_dsize_entry_is_unchanged(rz, hw, hw2):
    """The two entries share the kernel and its pixel arithmetic: the dsize form's outputs are still its restatement's, the exact 2x
    shrink (the 2 x 2 mean) included."""
    x = np.random.default_rng(hw[0] * 1000 + hw[1]).integers(0, 256, (3,) + hw + (3,), dtype=np.uint8)
    got = rz.resize_u8(torch.from_numpy(x), hw2[1], hw2[0]).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], R.resize_linear(x[i], hw2[1], hw2[0])), (hw, hw2, i)
