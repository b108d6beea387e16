"""GPU suite (-m gpu): the detector inputs of the sequence pre-pass resized on the device (KEEP_AMD_GPU_DETECT_RESIZE,
keep_processor.py:_prep_detect_chunk) with a helper that brings no resize of its own, on a machine without cv2: the batch the detector
receives is the numpy restatement of cv2.resize(INTER_AREA) (tests/cv_area_ref.py), and landmarks, detections and helper state equal a
run whose host resize is that restatement."""
import os
import sys

import numpy as np
import pytest
import torch

import cv_area_ref as R

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

H, W, RESIZE = 90, 160, 64
H2, W2 = 64, 113                                  # int(90 * 64 / 90), int(160 * 64 / 90)


@pytest.fixture(scope='module')
def detector():
    from comfyui_keep_amd.engine import retinaface as RF
    det = RF.EngineRetinaFace(RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0)).to('cuda'))
    det.engine.max_frames = 4
    return det


def make(detector, monkeypatch, knob):
    import types
    import synth_facehelper as SF
    from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor
    monkeypatch.setenv('KEEP_AMD_GPU_DETECT_RESIZE', knob)
    helper = SF.SynthFaceHelper(detector, None, (H, W), faces=2)
    helper.resize_for_detector = None             # a helper without a resize of its own, like the reference's
    pack = types.SimpleNamespace(keep_net=None, face_helper=helper, bg_upscale_model=None, face_upscale_model=None,
                                 device=torch.device('cuda'), model_type_str='KEEP')
    proc = KEEPFaceProcessor(pack)
    proc.detect_resize = RESIZE                   # (the pre-pass's 640, brought down to the size of these frames)
    return proc, helper


def video(n):
    return [f for f in np.random.default_rng(5).integers(0, 256, (n, H, W, 3), dtype=np.uint8)]


def test_prep_detect_chunk_returns_the_restatement_on_the_device(detector, monkeypatch):
    from comfyui_keep_amd.engine import hiplib as L
    proc, helper = make(detector, monkeypatch, '1')
    frames = video(5)
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    states, batch = proc._prep_detect_chunk(frames, RESIZE)
    assert calls == ['keep_resize_area_u8']                                    # one launch for the chunk
    assert isinstance(batch, torch.Tensor) and batch.is_cuda and batch.dtype == torch.uint8 and tuple(batch.shape) == (5, H2, W2, 3)
    assert proc.gpu_detect_resize is True                                      # (no failure turned the path off)
    ref = np.stack([R.resize_area(f, W2, H2) for f in frames])
    assert np.array_equal(batch.cpu().numpy(), ref)
    assert len(states) == 5 and all(s[0] is f and s[1] is False for s, f in zip(states, frames))


def test_detect_all_equals_a_run_with_the_restatement_as_the_host_resize(detector, monkeypatch):
    from comfyui_keep_amd.modules import keep_processor as KP
    frames = video(7)

    def run(knob):
        proc, helper = make(detector, monkeypatch, knob)
        seen = {'batches': [], 'results': [], 'states': []}
        real_batch = detector.engine.detect_batch

        def rec_batch(x, *a, **kw):
            out = real_batch(x, *a, **kw)
            seen['batches'].append((type(x).__name__, torch.as_tensor(x).cpu().numpy().copy()))
            seen['results'].append([np.array(r) for r in out])
            return out
        own = helper.get_face_landmarks_5

        def rec_landmarks(*a, **kw):
            seen['states'].append((helper.input_img, helper.is_gray))
            return own(*a, **kw)
        monkeypatch.setattr(detector.engine, 'detect_batch', rec_batch)
        monkeypatch.setattr(helper, 'get_face_landmarks_5', rec_landmarks)
        helper.begin_sequence()
        raw = proc._detect_all(frames, False)
        monkeypatch.setattr(detector.engine, 'detect_batch', real_batch)
        return raw, seen, proc

    raw_dev, dev, proc = run('1')
    assert proc.gpu_detect_resize is True
    monkeypatch.setattr(KP, '_resize', lambda img, w, h, interp: R.resize_area(img, w, h))
    raw_ref, ref, _ = run('0')

    assert [k for k, _ in dev['batches']] == ['Tensor', 'Tensor'] and [k for k, _ in ref['batches']] == ['ndarray', 'ndarray']
    assert [b.shape for _, b in dev['batches']] == [(4, H2, W2, 3), (3, H2, W2, 3)]
    for (_, a), (_, b) in zip(dev['batches'], ref['batches']):
        assert np.array_equal(a, b)                                            # the detector saw the same pixels
    for ra, rb in zip(dev['results'], ref['results']):
        assert len(ra) == len(rb) and all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(ra, rb))
    assert len(raw_dev) == len(raw_ref) == 7
    for fa, fb in zip(raw_dev, raw_ref):
        assert len(fa) == len(fb) == 2 and all(np.array_equal(np.asarray(p).view(np.uint64), np.asarray(q).view(np.uint64)) for p, q in zip(fa, fb))
    assert len(dev['states']) == len(ref['states']) == 7
    for (ia, ga), (ib, gb), f in zip(dev['states'], ref['states'], frames):
        assert ia is f and ib is f and ga is gb is False                       # input_img / is_gray as read_image left them
