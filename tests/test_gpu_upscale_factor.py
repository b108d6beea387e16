"""GPU suite (-m gpu): final_upscale_factor != 1 end to end through the product's entry points on a machine without cv2 -- the
background's INTER_LANCZOS4 resize runs on the device (engine/resize.py) and feeds the HIP paste.  The streamed sequence path
equals the per-frame path bit for bit (float node entry and process_frames_u8), pixels outside every pasted face's box equal the
numpy restatement of cv2.resize (tests/cv_lanczos_ref.py) of the input frame, and the aligned outputs are the restatement of the
restored faces."""
import os
import sys

import numpy as np
import pytest
import torch

import cv_lanczos_ref as R

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))


def _record_inverse_affines(helper):
    """Wrap the helper's get_inverse_affine: one list of crop -> output-frame matrices per call (= per pasted frame, in order)."""
    seen = []
    own = helper.get_inverse_affine

    def rec(*a, **kw):
        own(*a, **kw)
        seen.append([np.array(M) for M in helper.inverse_affine_matrices])
    helper.get_inverse_affine = rec
    return seen


def _outside_boxes(shape, mats):
    from comfyui_keep_amd.engine.paste import face_box
    H2, W2 = shape[:2]
    keep = np.ones((H2, W2), bool)
    for M in mats:
        x0, y0, x1, y1 = face_box(M, 512, 512, W2, H2)
        keep[y0:y1, x0:x1] = False
    return keep


@pytest.mark.parametrize('factor', [2.0, 0.7])
def test_sequence_upscale_factor_streamed_equals_per_frame_and_the_restatement(gpu_net, monkeypatch, factor):
    import synth_facehelper as SF
    from comfyui_keep_amd.modules.utils import comfy_image_to_cv2
    monkeypatch.delenv('KEEP_AMD_GPU_RESIZE', raising=False)
    H, W, faces, n = 360, 480, 2, 6
    H2, W2 = int(H * factor), int(W * factor)
    proc, helper = SF.make_processor(gpu_net, (H, W), faces)
    seen = _record_inverse_affines(helper)
    g = torch.Generator().manual_seed(7)
    frames = torch.rand((n, H, W, 3), generator=g)
    frames_u8 = [comfy_image_to_cv2(frames[i]) for i in range(n)]

    def run(stream, u8=False):
        monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', '1' if stream else '0')
        monkeypatch.setenv('KEEP_AMD_STREAM_GROUPS', '2')
        helper.begin_sequence()
        seen.clear()
        if u8:
            return proc.process_frames_u8(frames_u8, factor, False, False, False, max_clip_length=4)
        return proc.process_image_sequence(frames, factor, False, False, False, max_clip_length=4)

    ref = run(False)
    got = run(True)
    assert proc.gpu_resize is True                           # auto without cv2: the device path (with cv2: its self-check agreed)
    assert got.shape == ref.shape == (n, H2, W2, 3) and got.dtype == torch.float32
    assert torch.equal(got, ref)
    u8 = run(True, u8=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (n, H2, W2, 3)
    assert torch.equal(u8.flip(-1).float() / 255.0, ref)
    ref8 = run(False, u8=True)
    assert len(ref8) == n and all(np.array_equal(u8[i].numpy(), ref8[i]) for i in range(n))
    assert len(seen) == n and all(len(m) == faces for m in seen)
    pasted = 0
    for i in range(n):
        bg = R.resize_lanczos4(frames_u8[i], W2, H2)
        out = u8[i].numpy()
        keep = _outside_boxes(out.shape, seen[i])
        assert keep.sum() > 0.3 * keep.size
        assert np.array_equal(out[keep], bg[keep]), i
        pasted += int((out[~keep] != bg[~keep]).any(-1).sum())
    assert pasted > 1000                                     # (faces were really pasted)


def test_process_image_upscale_factor_2(gpu_net, monkeypatch):
    import synth_facehelper as SF
    monkeypatch.delenv('KEEP_AMD_GPU_RESIZE', raising=False)
    H, W, factor = 360, 480, 2.0
    proc, helper = SF.make_processor(gpu_net, (H, W), 2)
    seen = _record_inverse_affines(helper)
    img = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    helper.begin_sequence()
    out = proc.process_image(img, factor, False, False, False)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (int(H * factor), int(W * factor), 3)
    bg = R.resize_lanczos4(img, int(W * factor), int(H * factor))
    assert len(seen) == 1 and len(seen[0]) == 2
    keep = _outside_boxes(out.shape, seen[0])
    assert np.array_equal(out[keep], bg[keep])
    assert int((out[~keep] != bg[~keep]).any(-1).sum()) > 1000


def test_aligned_outputs_are_the_restatement_of_the_restored_faces(gpu_net, monkeypatch):
    """return_restored_aligned (sequence) and process_image(has_aligned=True): the restored 512 x 512 face resized to
    512 * factor on the device.  (Aligned inputs are 512 x 512 already: their INTER_LINEAR resize to 512 is the identity.)"""
    import synth_facehelper as SF
    monkeypatch.delenv('KEEP_AMD_GPU_RESIZE', raising=False)
    monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', '0')
    factor, side = 2.0, 1024
    proc, helper = SF.make_processor(gpu_net, (512, 512), 1)
    proc.return_restored_aligned = True
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (512, 512, 3), dtype=np.uint8) for _ in range(3)]
    outs = proc.process_frames_u8(frames, factor, True, False, False, max_clip_length=4)
    faces = [np.asarray(f) for f in proc.last_restored_faces]
    assert len(outs) == len(faces) == 3
    for o, f in zip(outs, faces):
        assert isinstance(o, np.ndarray) and o.shape == (side, side, 3)
        assert np.array_equal(o, R.resize_lanczos4(f, side, side))
    one = proc.process_image(frames[0], factor, True, False, False)
    assert one.shape == (side, side, 3)
    assert np.array_equal(one, R.resize_lanczos4(np.asarray(proc.last_restored_faces[0]), side, side))
