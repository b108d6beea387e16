"""GPU suite (-m gpu): aligned inputs that are not 512 x 512, end to end through the product's entry points on a machine without cv2 --
the INTER_LINEAR resize to 512 x 512 runs on the device (engine/resize.py:LinearResizer), and an aligned sequence stays there
(``_aligned_streamed``): its result equals the per-frame path's bit for bit and the numpy restatements of both resizes
(tests/cv_linear_ref.py, tests/cv_lanczos_ref.py) around a direct ``run_clips_u8``."""
import os
import sys

import numpy as np
import pytest
import torch

import cv_lanczos_ref as RL
import cv_linear_ref as R

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

H, W, N, CLIP = 96, 128, 5, 2


def _setup(gpu_net, monkeypatch, knob=None):
    """(processor, float IMAGE frames, the same frames as uint8 BGR); ``knob``: KEEP_AMD_GPU_ALIGNED_RESIZE while the processor is made."""
    import synth_facehelper as SF
    from comfyui_keep_amd.modules.utils import comfy_image_to_cv2
    for k in ('KEEP_AMD_GPU_RESIZE', 'KEEP_AMD_GPU_ALIGNED_RESIZE', 'KEEP_AMD_STREAM_GROUPS', 'KEEP_AMD_DETECT_BATCH'):
        monkeypatch.delenv(k, raising=False)
    if knob is not None:
        monkeypatch.setenv('KEEP_AMD_GPU_ALIGNED_RESIZE', knob)
    proc, helper = SF.make_processor(gpu_net, (H, W), 1)
    proc.keep_restored_faces = True
    frames = torch.rand((N, H, W, 3), generator=torch.Generator().manual_seed(11))
    frames_u8 = [comfy_image_to_cv2(frames[i]) for i in range(N)]
    return proc, frames, frames_u8


def _record_launches(monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def _direct_restore(gpu_net, frames_u8):
    """The restored crops of the sequence from the restated resize and the net alone: clips of CLIP crops, the last one a single frame."""
    crops = np.stack([R.resize_linear(f, 512, 512) for f in frames_u8])
    outs = gpu_net.run_clips_u8([crops[s:s + CLIP] for s in range(0, N, CLIP)])
    return np.concatenate([o.numpy() for o in outs])


def test_default_aligned_sequence_at_factor_2(gpu_net, monkeypatch):
    """Reference quirk P2: the output is the input frame at the output size; the restored faces are computed and kept on request."""
    proc, frames, frames_u8 = _setup(gpu_net, monkeypatch)
    calls = _record_launches(monkeypatch)
    monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', '0')
    ref = proc.process_frames_u8(frames_u8, 2.0, True, False, False, max_clip_length=CLIP)
    ref_faces = [np.asarray(f) for f in proc.last_restored_faces]
    assert isinstance(ref, list) and len(ref) == N and calls.count('keep_resize_linear_u8') == N      # one launch per frame
    calls.clear()
    monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', '1')
    got = proc.process_frames_u8(frames_u8, 2.0, True, False, False, max_clip_length=CLIP)
    assert calls.count('keep_resize_linear_u8') == 1                                                   # one launch per chunk
    assert proc.gpu_aligned_resize is True and proc.gpu_resize is True
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and tuple(got.shape) == (N, 2 * H, 2 * W, 3)
    faces = [np.asarray(f) for f in proc.last_restored_faces]
    direct = _direct_restore(gpu_net, frames_u8)
    assert len(faces) == len(ref_faces) == N
    for i in range(N):
        assert np.array_equal(got[i].numpy(), ref[i]), i
        assert np.array_equal(ref[i], RL.resize_lanczos4(frames_u8[i], 2 * W, 2 * H)), i
        assert faces[i].shape == (512, 512, 3) and np.array_equal(faces[i], ref_faces[i]), i
        assert np.array_equal(faces[i], direct[i]), i
    assert len({f.tobytes() for f in faces}) == N                                                      # (five different faces)
    # the float entry: the same frames as ComfyUI's RGB floats
    seq = proc.process_image_sequence(frames, 2.0, True, False, False, max_clip_length=CLIP)
    assert seq.dtype == torch.float32 and torch.equal(seq, got.flip(-1).float() / 255.0)
    # without keep_restored_faces nothing of the sequence is kept
    proc.keep_restored_faces = False
    again = proc.process_frames_u8(frames_u8, 2.0, True, False, False, max_clip_length=CLIP)
    assert torch.equal(again, got) and len(proc.last_restored_faces) == 0


def test_return_restored_aligned_at_factor_1_5(gpu_net, monkeypatch):
    proc, frames, frames_u8 = _setup(gpu_net, monkeypatch)
    proc.return_restored_aligned = True
    side = int(512 * 1.5)
    monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', '0')
    ref = proc.process_frames_u8(frames_u8, 1.5, True, False, False, max_clip_length=CLIP)
    monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', '1')
    got = proc.process_frames_u8(frames_u8, 1.5, True, False, False, max_clip_length=CLIP)
    faces = [np.asarray(f) for f in proc.last_restored_faces]
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and tuple(got.shape) == (N, side, side, 3)
    assert isinstance(ref, list) and len(ref) == len(faces) == N
    for i in range(N):
        assert np.array_equal(got[i].numpy(), ref[i]), i
        assert np.array_equal(ref[i], RL.resize_lanczos4(faces[i], side, side)), i
    seq = proc.process_image_sequence(frames, 1.5, True, False, False, max_clip_length=CLIP)
    assert seq.dtype == torch.float32 and tuple(seq.shape) == (N, side, side, 3)
    assert torch.equal(seq, got.flip(-1).float() / 255.0)


def test_process_image_takes_an_aligned_input_of_any_size(gpu_net, monkeypatch):
    proc, frames, frames_u8 = _setup(gpu_net, monkeypatch)
    out = proc.process_image(frames_u8[0], 1.0, True, False, False)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (512, 512, 3)
    crop = R.resize_linear(frames_u8[0], 512, 512)
    assert np.array_equal(out, gpu_net.run_clips_u8([crop[None]])[0][0].numpy())
    assert np.array_equal(out, np.asarray(proc.last_restored_faces[0]))


def test_the_knob_turned_off_without_cv2_raises_as_before(gpu_net, monkeypatch):
    from comfyui_keep_amd.modules import keep_processor as KP
    proc, frames, frames_u8 = _setup(gpu_net, monkeypatch, knob='0')
    monkeypatch.setattr(KP, '_cv2', lambda: (_ for _ in ()).throw(ImportError('no cv2')))
    assert proc.gpu_aligned_resize is False
    for stream in ('1', '0'):
        monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', stream)
        with pytest.raises(ImportError):
            proc.process_frames_u8(frames_u8, 1.0, True, False, False, max_clip_length=CLIP)
    with pytest.raises(ImportError):
        proc.process_image(frames_u8[0], 1.0, True, False, False)


def test_a_failing_device_resize_in_the_streamed_form_falls_back(gpu_net, monkeypatch):
    """... it is logged, turns the path off, and the per-frame path takes the sequence -- which without cv2 raises as above."""
    from comfyui_keep_amd.modules import keep_processor as KP
    proc, frames, frames_u8 = _setup(gpu_net, monkeypatch)
    monkeypatch.setattr(KP, '_cv2', lambda: (_ for _ in ()).throw(ImportError('no cv2')))
    monkeypatch.setattr(proc, '_aligned_resize_device', lambda *a, **k: (_ for _ in ()).throw(RuntimeError('launch failed')))
    monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', '1')
    with pytest.raises(ImportError):
        proc.process_frames_u8(frames_u8, 1.0, True, False, False, max_clip_length=CLIP)
    assert proc.gpu_aligned_resize is False
