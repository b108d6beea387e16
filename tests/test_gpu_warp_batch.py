"""GPU suite (-m gpu): keep_warp_affine_batch_u8 (csrc/keep_paste.hip) -- the aligned crops of F faces from N resident frames in one call --
bit for bit against the single-frame kernel keep_warp_affine_u8 on the same frame and map, and against the numpy restatement
(tests/flat_ref.py:ref_warp_affine over oracle/paste_oracle.py); the boundary between two launches; the bytes it touches; and that the
frame index matters."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import flat_ref
import footprint as FP
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import paste

pytestmark = pytest.mark.gpu

N, H, W, DH, DW = 3, 37, 53, 24, 40
_C, _S = 0.7 * math.cos(0.6), 0.7 * math.sin(0.6)
# (frame, destination -> source map)
FACES = [(0, [1.0, 0.0, 3.25, 0.0, 1.0, 2.5]),
         (0, [0.8, 0.0, 1.1, 0.0, 0.8, 4.3]),                      # a second face of the same frame
         (1, [1.5, 0.0, -10.3, 0.0, 1.5, -7.7]),                   # hangs over the top and the left edge: reads the border colour
         (1, [_C, -_S, 20.2, _S, _C, 5.1]),                        # rotated by 0.6 rad at scale 0.7
         (-1, [0.0] * 6),                                          # the black crop
         (2, [1.0, 0.0, 5.0, 0.0, 1.0, 7.0])]                      # the last frame, landing exactly on whole pixels


@pytest.fixture(scope='module')
def frames():
    return torch.from_numpy(np.random.default_rng(11).integers(0, 256, (N, H, W, 3), dtype=np.uint8))


def batch(src, faces, dh, dw, border, dst=None):
    """One keep_warp_affine_batch_u8 call on the faces [(frame, six doubles)] -> uint8 [F,dh,dw,3] on the device."""
    F = len(faces)
    if dst is None:
        dst = torch.full((F, dh, dw, 3), 0xA5, dtype=torch.uint8, device='cuda')
    idx = (C.c_int32 * F)(*[f for f, _ in faces])
    d2s = (C.c_double * (6 * F))(*[v for _, m in faces for v in m])
    n, h, w, _ = src.shape
    L.call('keep_warp_affine_batch_u8', src, n, h, w, dst, F, dh, dw, idx, d2s, *border)
    return dst


def single(frame, m, dh, dw, border):
    out = torch.empty((dh, dw, 3), dtype=torch.uint8, device='cuda')
    L.call('keep_warp_affine_u8', frame, frame.shape[0], frame.shape[1], out, dh, dw, (C.c_double * 6)(*m), *border)
    return out


@pytest.mark.parametrize('border', [(135, 133, 132), (7, 250, 91)])
def test_every_face_equals_the_single_frame_kernel_and_the_restatement(frames, border):
    src = frames.cuda()
    got = batch(src, FACES, DH, DW, border)
    torch.cuda.synchronize()
    for i, (f, m) in enumerate(FACES):
        if f < 0:
            assert not got[i].any()                                # all zeros
            continue
        assert torch.equal(got[i], single(src[f], m, DH, DW, border)), i
        ref = flat_ref.ref_warp_affine(dict(h=H, w=W, dh=DH, dw=DW, m=m, border=list(border)), {'src': frames[f].reshape(H * W, 3)})['dst']
        assert ref['kind'] == 'exact' and torch.equal(got[i].cpu().reshape(DH * DW, 3), ref['ref']), i
    bc = torch.tensor(border, dtype=torch.uint8, device='cuda')
    assert (got[2] == bc).all(-1).any() and not (got[2] == bc).all()            # the border colour is in the overhanging crop
    assert torch.equal(got[5], src[2][7:7 + DH, 5:5 + DW])                      # whole pixels: a plain copy
    assert not torch.equal(got[0], got[1])


def test_the_python_wrapper_equals_crop_faces_and_calls_the_library_once(frames, monkeypatch):
    """``crop_faces_batch`` takes the frame -> crop matrices ``crop_faces`` takes (None: the black crop) and writes into a slice."""
    src = frames.cuda()
    fwd = [paste.invert_affine(np.array(m, np.float64).reshape(2, 3)) if f >= 0 else None for f, m in FACES]
    frame_of = [max(f, 0) for f, _ in FACES]
    out = torch.full((len(FACES) + 2, DH, DW, 3), 0xA5, dtype=torch.uint8, device='cuda')
    calls, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    res = paste.crop_faces_batch(src, frame_of, fwd, out[1:-1], (DW, DH))
    assert calls == ['keep_warp_affine_batch_u8'] and res.data_ptr() == out[1].data_ptr()
    monkeypatch.setattr(L, 'call', real)
    for i, (f, _) in enumerate(FACES):
        assert torch.equal(out[1 + i], paste.crop_faces(frames[max(f, 0)], [fwd[i]], (DW, DH))[0]), i
    assert (out[0] == 0xA5).all() and (out[-1] == 0xA5).all()
    with pytest.raises(ValueError):
        paste.crop_faces_batch(src, frame_of[:-1], fwd, out[1:-1], (DW, DH))
    with pytest.raises(ValueError):
        paste.crop_faces_batch(src, frame_of, fwd, out[1:], (DW, DH))
    with pytest.raises(L.KeepHipError, match='keep_warp_affine_batch_u8'):
        paste.crop_faces_batch(src, [N] * len(fwd), [np.eye(2, 3)] * len(fwd), out[1:-1], (DW, DH))
    torch.cuda.synchronize()


def test_the_second_launch_starts_at_face_32(monkeypatch):
    """F = 33 faces are two launches inside ONE library call; face 32, the first of the second launch, is its single-face result."""
    rng = np.random.default_rng(3)
    src = torch.from_numpy(rng.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8)).cuda()
    faces = [(i % 2, [1.0, 0.0, 0.25 * i - 2.0, 0.0, 1.0, 0.125 * i]) for i in range(33)]
    calls, real = [], L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = batch(src, faces, 8, 8, (135, 133, 132))
    assert calls == ['keep_warp_affine_batch_u8']
    monkeypatch.setattr(L, 'call', real)
    for i in (0, 31, 32):
        assert torch.equal(got[i], single(src[faces[i][0]], faces[i][1], 8, 8, (135, 133, 132))), i
    assert not torch.equal(got[32], got[31]) and not (got == 0xA5).all(-1).all(-1).all(-1).any()      # every crop was written


def test_footprint_only_the_crops_are_written_and_the_source_is_left_alone(frames):
    """Source and destination inside larger buffers of a known pattern: no byte outside [F,dh,dw,3] changes, nothing outside the frames
    reaches a result, and the frames -- frame 1, which no face refers to, included -- are what they were."""
    faces = [(0, FACES[0][1]), (2, FACES[2][1]), (-1, [0.0] * 6), (2, FACES[3][1])]
    F = len(faces)
    regions = [FP.single('src', frames.reshape(N * H * W, 3), role='r'),
               FP.output('dst', (F * DH * DW, 3), dtype=torch.uint8)]

    def launch(t):
        src = t['src']
        assert src.is_contiguous() and t['dst'].is_contiguous()
        before = src.clone()
        batch(src.view(N, H, W, 3), faces, DH, DW, (135, 133, 132), dst=t['dst'].view(F, DH, DW, 3))
        torch.cuda.synchronize()
        assert torch.equal(src, before)
    out = FP.run(launch, regions, 'cuda')['dst'].view(F, DH, DW, 3)
    assert torch.equal(out, batch(frames.cuda(), faces, DH, DW, (135, 133, 132)))


def test_the_frame_index_matters(frames):
    src = frames.cuda()
    live = [fm for fm in FACES if fm[0] >= 0]
    got = batch(src, live, DH, DW, (135, 133, 132))
    moved = [((f + 1) % N, m) for f, m in live]
    other = batch(src, moved, DH, DW, (135, 133, 132))
    for i in range(len(live)):
        assert not torch.equal(got[i], other[i]), i
        assert torch.equal(other[i], single(src[moved[i][0]], moved[i][1], DH, DW, (135, 133, 132))), i
