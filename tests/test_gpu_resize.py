"""GPU suite (-m gpu): keep_resize_lanczos4_u8 (csrc/keep_resize.hip, through engine/resize.py) bit for bit against the independent
numpy restatement of cv2.resize(INTER_LANCZOS4) (tests/cv_lanczos_ref.py)."""
import numpy as np
import pytest
import torch

import cv_lanczos_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rz():
    from comfyui_keep_amd.engine.resize import Lanczos4Resizer
    return Lanczos4Resizer('cuda')


def frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def check(rz, img, w2, h2):
    got = rz.resize_u8(img, w2, h2)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (h2, w2, 3)
    ref = R.resize_lanczos4(img, w2, h2)
    got = got.cpu().numpy()
    assert np.array_equal(got, ref), (img.shape, (h2, w2), np.argwhere(got != ref)[:4])


def test_1080p_to_2160p_and_720p_at_1_3(rz):
    check(rz, frame(1080, 1920, 0), 3840, 2160)
    check(rz, frame(720, 1280, 1), int(1280 * 1.3), int(720 * 1.3))


@pytest.mark.parametrize('f', [0.5, 0.7, 4.0])
def test_small_frames_down_and_up(rz, f):
    img = frame(120, 160, 2)
    check(rz, img, int(160 * f), int(120 * f))


@pytest.mark.parametrize('hw,hw2', [((37, 53), (48, 69)), ((101, 67), (50, 33)), ((300, 9), (100, 3)), ((9, 300), (3, 100)),
                                     ((31, 17), (15, 1)), ((7, 40), (1, 13)), ((1, 1), (5, 5)), ((2, 3), (7, 11)),
                                     ((64, 2000), (64, 3)), ((33, 35), (33, 70))])
def test_odd_sizes_whole_pixel_coordinates_and_one_pixel_outputs(rz, hw, hw2):
    (h, w), (h2, w2) = hw, hw2
    check(rz, frame(h, w, h * 1000 + w), w2, h2)


def test_three_frames_in_one_launch_equal_their_single_frame_results(rz, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    frames = np.stack([frame(90, 130, 10 + i) for i in range(3)])
    frames[1] = 255 - frames[1]
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = rz.resize_u8(torch.from_numpy(frames), 260, 180)
    assert calls == ['keep_resize_lanczos4_u8'] and tuple(got.shape) == (3, 180, 260, 3)
    for i in range(3):
        one = rz.resize_u8(frames[i], 260, 180)
        assert torch.equal(got[i], one)
        assert np.array_equal(got[i].cpu().numpy(), R.resize_lanczos4(frames[i], 260, 180))


def test_identity_launches_nothing(rz, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    monkeypatch.setattr(L, 'call', lambda *a: pytest.fail(f"launched {a[0]}"))
    img = frame(40, 50, 3)
    assert rz.resize_u8(img, 50, 40) is img
    t = torch.from_numpy(np.stack([img, img]))
    assert rz.resize_u8(t, 50, 40) is t


def test_bad_arguments_fail_loudly(rz):
    from comfyui_keep_amd.engine import hiplib as L
    lib = L.load()
    x = torch.zeros((8, 8, 3), dtype=torch.uint8, device='cuda')
    y = torch.zeros((16, 16, 3), dtype=torch.uint8, device='cuda')
    o = torch.zeros(16, dtype=torch.int32, device='cuda')
    c = torch.zeros((16, 8), dtype=torch.int16, device='cuda')
    args = [x.data_ptr(), y.data_ptr(), 1, 8, 8, 16, 16, o.data_ptr(), c.data_ptr(), o.data_ptr(), c.data_ptr(), None]
    for i, bad in ((0, None), (1, None), (7, None), (10, None), (2, 0), (3, 0), (4, -1), (5, 0), (6, -3), (4, 1 << 30),
                   (6, (1 << 30) + 5)):
        a = list(args)
        a[i] = bad
        assert lib.keep_resize_lanczos4_u8(*a) == -1, (i, bad)
        assert lib.keep_last_error().startswith(b'keep_resize_lanczos4_u8'), lib.keep_last_error()
    with pytest.raises(L.KeepHipError, match='keep_resize_lanczos4_u8'):
        L.call('keep_resize_lanczos4_u8', x, y, 0, 8, 8, 16, 16, o, c, o, c)
    with pytest.raises(ValueError):
        rz.resize_u8(np.zeros((8, 8), np.uint8), 16, 16)
    assert lib.keep_resize_lanczos4_u8(*args) == 0                       # (the well-formed call runs)
    torch.cuda.synchronize()
