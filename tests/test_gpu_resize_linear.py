"""GPU suite (-m gpu): keep_resize_linear_u8 (csrc/keep_resize_linear.hip, through engine/resize.py) bit for bit against the independent
numpy restatement of cv2.resize(INTER_LINEAR) (tests/cv_linear_ref.py) -- enlargements, shrinks on both sides of the staged / unstaged
threshold, the exact 2x shrink, one-row, one-column and one-pixel cases -- and four cases in poisoned surroundings (tests/footprint.py)."""
import numpy as np
import pytest
import torch

import cv_linear_ref as R
import footprint as FP

pytestmark = pytest.mark.gpu

# (H, W) -> (H2, W2)
GEOMETRIES = [((23, 31), (64, 64)),        # enlarge, non-square source, several tiles
              ((90, 120), (64, 64)),       # fractional shrink below 2
              ((128, 96), (64, 48)),       # exact 2x
              ((130, 96), (64, 48)),       # 2x on x only, so the general case
              ((600, 800), (64, 64)),      # large shrink, sparse footprint (nothing staged)
              ((1, 9), (4, 20)),           # one source row
              ((9, 1), (20, 4)),           # one source column
              ((5, 7), (1, 1)),            # one output pixel
              ((256, 256), (512, 512))]    # a product geometry


@pytest.fixture(scope='module')
def rz():
    from comfyui_keep_amd.engine.resize import LinearResizer
    return LinearResizer('cuda')


_REF = {}


def reference(hw, hw2):
    """(frames [3,H,W,3], restatement [3,H2,W2,3]) of a geometry: computed once, shared, never written to."""
    key = (hw, hw2)
    if key not in _REF:
        x = np.random.default_rng(hw[0] * 1000 + hw[1]).integers(0, 256, (3,) + hw + (3,), dtype=np.uint8)
        ref = np.stack([R.resize_linear(f, hw2[1], hw2[0]) for f in x])
        x.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (x, ref)
    return _REF[key]


@pytest.mark.parametrize('hw,hw2', GEOMETRIES)
def test_three_random_frames_equal_the_restatement(rz, hw, hw2):
    x, ref = reference(hw, hw2)
    got = rz.resize_u8(torch.from_numpy(x.copy()), hw2[1], hw2[0])
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (3, hw2[0], hw2[1], 3)
    got = got.cpu().numpy()
    print(f"{hw} -> {hw2}: {int((got != ref).sum())} of {ref.size} values differ from the restatement")
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:4]


@pytest.mark.parametrize('hw,hw2', GEOMETRIES)
def test_constant_frames_stay_constant(rz, hw, hw2):
    for value in (255, 0):
        x = np.full(hw + (3,), value, np.uint8)
        got = rz.resize_u8(x, hw2[1], hw2[0])
        assert tuple(got.shape) == (hw2[0], hw2[1], 3) and bool((got == value).all()), value


def test_batched_equals_one_by_one_in_one_launch(rz, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    x, ref = reference((90, 120), (64, 64))
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = rz.resize_u8(x.copy(), 64, 64)
    assert calls == ['keep_resize_linear_u8']
    for i in range(3):
        one = rz.resize_u8(x[i].copy(), 64, 64)
        assert tuple(one.shape) == (64, 64, 3) and torch.equal(got[i], one)
    into = torch.full((5, 64, 64, 3), 7, dtype=torch.uint8, device='cuda')           # out=: a slice of a larger batch
    assert rz.resize_u8(x.copy(), 64, 64, out=into[1:4]).data_ptr() == into[1].data_ptr()
    assert torch.equal(into[1:4], got) and bool((into[0] == 7).all()) and bool((into[4] == 7).all())


def test_identity_returns_the_input_and_launches_nothing(rz, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    monkeypatch.setattr(L, 'call', lambda *a: pytest.fail(f"launched {a[0]}"))
    x = torch.zeros((2, 9, 11, 3), dtype=torch.uint8, device='cuda')
    assert rz.resize_u8(x, 11, 9) is x
    img = np.zeros((9, 11, 3), np.uint8)
    assert rz.resize_u8(img, 11, 9) is img


def test_identity_geometry_through_the_kernel_is_an_exact_copy():
    """The launcher has no special case for identity: the arithmetic gives weights (2048, 0) and the value itself."""
    from comfyui_keep_amd.engine import hiplib as L
    x = torch.randint(0, 256, (2, 19, 70, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    y = torch.zeros_like(x)
    L.call('keep_resize_linear_u8', x, y, 2, 19, 70, 19, 70)
    assert torch.equal(x, y)


def test_empty_batches_and_bad_arguments_launch_nothing(rz, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    lib = L.load()
    x = torch.zeros((1, 90, 120, 3), dtype=torch.uint8, device='cuda')
    y = torch.full((1, 64, 64, 3), 7, dtype=torch.uint8, device='cuda')
    with pytest.raises(L.KeepHipError, match='keep_resize_linear_u8'):
        L.call('keep_resize_linear_u8', x, y, 0, 90, 120, 64, 64)                             # N = 0
    args = [x.data_ptr(), y.data_ptr(), 1, 90, 120, 64, 64, None]
    for i, bad in ((0, None), (1, None), (2, -1), (2, 70000), (3, 0), (4, -2), (5, 0), (6, 0), (4, 1 << 30), (6, 1 << 30)):
        a = list(args)
        a[i] = bad
        assert lib.keep_resize_linear_u8(*a) == -1, (i, bad)
        assert lib.keep_last_error().startswith(b'keep_resize_linear_u8'), lib.keep_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7).all())                                                                 # nothing ran
    with pytest.raises(ValueError):
        rz.resize_u8(np.zeros((90, 120), np.uint8), 64, 64)
    with pytest.raises(ValueError):
        rz.resize_u8(np.zeros((90, 120, 3), np.float32), 64, 64)
    monkeypatch.setattr(L, 'call', lambda *a: pytest.fail(f"launched {a[0]}"))
    empty = rz.resize_u8(torch.zeros((0, 90, 120, 3), dtype=torch.uint8), 64, 64)
    assert tuple(empty.shape) == (0, 64, 64, 3) and empty.is_cuda


def _linear_case(n, h, w, h2, w2, unaligned):
    from comfyui_keep_amd.engine import hiplib as L
    g = torch.Generator().manual_seed(h * 1000 + w)
    src = torch.randint(0, 256, (n * h * w, 3), generator=g, dtype=torch.uint8)
    regions = FP.unaligned_u8(src, n * h2 * w2 * 3) if unaligned else [FP.single('src', src), FP.output('dst', (n * h2 * w2, 3), torch.uint8)]

    def launch(t):
        assert (t['src'].data_ptr() % 16, t['dst'].data_ptr() % 16) == ((5, 11) if unaligned else (0, 0))
        L.call('keep_resize_linear_u8', t['src'], t['dst'], n, h, w, h2, w2)
    return src, regions, launch


@pytest.mark.parametrize('case,n,hw,hw2', [('ragged', 3, (7, 101), (5, 67)), ('one_row', 1, (3, 75), (1, 44)), ('half', 1, (10, 14), (5, 7)),
                                           ('unstaged', 2, (40, 300), (3, 20)), ('unaligned', 3, (7, 101), (5, 67))])
def test_footprint_in_poisoned_surroundings(case, n, hw, hw2):
    """Every buffer of the launch sits between guards the test owns: nothing outside the payloads is written, nothing outside them reaches
    the result, and the result is the restatement's.  ('unstaged': a 15x shrink, whose tiles read global memory directly; 'unaligned': the
    launch's src and dst start 5 and 11 bytes into a 16-byte word.)"""
    (h, w), (h2, w2) = hw, hw2
    src, regions, launch = _linear_case(n, h, w, h2, w2, case == 'unaligned')
    out = FP.run(launch, regions, 'cuda')['dst'].cpu().numpy().reshape(n, h2, w2, 3)
    x = src.numpy().reshape(n, h, w, 3)
    for i in range(n):
        assert np.array_equal(out[i], R.resize_linear(x[i], w2, h2)), (case, i)
