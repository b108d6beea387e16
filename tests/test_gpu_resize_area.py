"""GPU suite (-m gpu): keep_resize_area_u8 (csrc/keep_resize_area.hip, through engine/resize.py) bit for bit against the independent
numpy restatement of cv2.resize(INTER_AREA) (tests/cv_area_ref.py), including a guard that a build with FMA contraction would not
pass, and two cases in poisoned surroundings (tests/footprint.py)."""
import numpy as np
import pytest
import torch

import cv_area_ref as R
import footprint as FP

pytestmark = pytest.mark.gpu

# (H, W) -> (H2, W2): 2-3 taps; scale < 1.2; a whole-number scale on y with a fractional one on x; more than one tile on both axes
GEOMETRIES = [((54, 96), (32, 56)), ((45, 80), (40, 71)), ((48, 64), (16, 21)), ((270, 480), (160, 284))]
CONTRACTION_SEED = 0       # a seed at which the (270, 480) frame tells fused from separate roundings (asserted below, on the CPU)


@pytest.fixture(scope='module')
def rz():
    from comfyui_keep_amd.engine.resize import AreaResizer
    return AreaResizer('cuda')


def frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


_REF = {}


def reference(hw, hw2):
    """(frames [3,H,W,3], restatement [3,H2,W2,3]) of a geometry: computed once, shared, never written to."""
    key = (hw, hw2)
    if key not in _REF:
        x = frames(3, *hw, seed=CONTRACTION_SEED if hw == (270, 480) else hw[0] * 1000 + hw[1])
        ref = np.stack([R.resize_area(f, hw2[1], hw2[0]) for f in x])
        x.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (x, ref)
    return _REF[key]


@pytest.mark.parametrize('hw,hw2', GEOMETRIES)
def test_three_random_frames_equal_the_restatement(rz, hw, hw2):
    x, ref = reference(hw, hw2)
    if hw == (270, 480):
        # the teeth of this case: on this very image a fused multiply-add changes at least one output value, so a contracted build fails below
        fused = R.resize_area(x[0], hw2[1], hw2[0], fused=True)
        n_diff = int((fused != ref[0]).sum())
        print(f"fused-emulating restatement differs from the plain one in {n_diff} of {fused.size} values")
        assert n_diff >= 1, "choose another CONTRACTION_SEED: this image does not tell a contracted build from a correct one"
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
    x, ref = reference((54, 96), (32, 56))
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = rz.resize_u8(x.copy(), 56, 32)
    assert calls == ['keep_resize_area_u8']
    for i in range(3):
        one = rz.resize_u8(x[i].copy(), 56, 32)
        assert tuple(one.shape) == (32, 56, 3) and torch.equal(got[i], one)


def test_empty_batches_and_bad_arguments_launch_nothing(rz, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    lib = L.load()
    x = torch.zeros((1, 54, 96, 3), dtype=torch.uint8, device='cuda')
    y = torch.full((1, 32, 56, 3), 7, dtype=torch.uint8, device='cuda')
    tables = rz._device_tables(54, 96, 32, 56)
    with pytest.raises(L.KeepHipError, match='keep_resize_area_u8'):
        L.call('keep_resize_area_u8', x, y, 0, 54, 96, 32, 56, *tables)                       # N = 0
    args = [x.data_ptr(), y.data_ptr(), 1, 54, 96, 32, 56] + [t.data_ptr() for t in tables] + [None]
    for i, bad in ((0, None), (1, None), (7, None), (12, None), (2, -1), (3, 0), (5, 54), (6, 96), (6, 200), (4, 1 << 30)):
        a = list(args)
        a[i] = bad
        assert lib.keep_resize_area_u8(*a) == -1, (i, bad)
        assert lib.keep_last_error().startswith(b'keep_resize_area_u8'), lib.keep_last_error()
    a = list(args)
    a[3:7] = [64, 96, 32, 48]                                                                   # scale 2 on both axes
    assert lib.keep_resize_area_u8(*a) == -1 and b'whole-number' in lib.keep_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7).all())                                                                 # nothing ran
    with pytest.raises(L.KeepHipError):
        rz.resize_u8(torch.zeros((64, 96, 3), dtype=torch.uint8), 48, 32)
    with pytest.raises(L.KeepHipError):
        rz.resize_u8(torch.zeros((64, 96, 3), dtype=torch.uint8), 96, 32)
    with pytest.raises(ValueError):
        rz.resize_u8(np.zeros((54, 96), np.uint8), 56, 32)
    with pytest.raises(ValueError):
        rz.resize_u8(np.zeros((54, 96, 3), np.float32), 56, 32)
    monkeypatch.setattr(L, 'call', lambda *a: pytest.fail(f"launched {a[0]}"))
    empty = rz.resize_u8(torch.zeros((0, 54, 96, 3), dtype=torch.uint8), 56, 32)
    assert tuple(empty.shape) == (0, 32, 56, 3) and empty.is_cuda


def _area_case(n, h, w, h2, w2, unaligned):
    from comfyui_keep_amd.engine import hiplib as L
    from comfyui_keep_amd.engine.resize import area_tables
    g = torch.Generator().manual_seed(h * 1000 + w)
    src = torch.randint(0, 256, (n * h * w, 3), generator=g, dtype=torch.uint8)
    (xs, xi, xa), (ys, yi, ya) = area_tables(w, w2), area_tables(h, h2)
    row = lambda a: torch.from_numpy(a).reshape(1, -1)
    regions = FP.unaligned_u8(src, n * h2 * w2 * 3) if unaligned else [FP.single('src', src), FP.output('dst', (n * h2 * w2, 3), torch.uint8)]
    regions += [FP.single('xs', row(xs)), FP.single('xi', row(xi)), FP.single('xa', row(xa)),
                FP.single('ys', row(ys)), FP.single('yi', row(yi)), FP.single('ya', row(ya))]

    def launch(t):
        assert (t['src'].data_ptr() % 16, t['dst'].data_ptr() % 16) == ((5, 11) if unaligned else (0, 0))
        L.call('keep_resize_area_u8', t['src'], t['dst'], n, h, w, h2, w2, t['xs'], t['xi'], t['xa'], t['ys'], t['yi'], t['ya'])
    return src, regions, launch


@pytest.mark.parametrize('case,n,hw,hw2', [('ragged', 3, (7, 101), (5, 67)), ('one_row', 1, (3, 75), (1, 44)), ('tiles', 2, (45, 80), (40, 71)),
                                           ('unaligned', 3, (7, 101), (5, 67))])
def test_footprint_in_poisoned_surroundings(case, n, hw, hw2):
    """Every buffer of the launch sits between guards the test owns: nothing outside the payloads is written, nothing outside them reaches
    the result, and the result is the restatement's.  ('unaligned': the launch's src and dst start 5 and 11 bytes into a 16-byte word.)"""
    (h, w), (h2, w2) = hw, hw2
    src, regions, launch = _area_case(n, h, w, h2, w2, case == 'unaligned')
    out = FP.run(launch, regions, 'cuda')['dst'].cpu().numpy().reshape(n, h2, w2, 3)
    x = src.numpy().reshape(n, h, w, 3)
    for i in range(n):
        assert np.array_equal(out[i], R.resize_area(x[i], w2, h2)), (case, i)
