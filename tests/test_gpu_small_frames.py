"""GPU suite (-m gpu): sequences and single images whose short side is below 512, with a helper whose ``read_image`` enlarges them the way
face_restoration_helper.py:182-184 does (modules/keep_processor.py: the small-frame form of ``_FrameStore``, the background resize of the
streamed paste without a store, ``_paste``).  Built on the ``Rig`` of tests/test_gpu_frame_store.py: the product's own entry points over
tools/synth_facehelper.py, the library calls, detector batches and paste backgrounds recorded.  The helper here enlarges with the numpy
restatement (tests/cv_linear_fxy_ref.py), so every equality below also holds the kernel to it."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import cv_lanczos_ref as RL
import cv_linear_fxy_ref as F
from test_gpu_frame_store import WARP, WARP_BATCH, Rig, net, video  # noqa: F401  (``net``: the module's fixture)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

ENLARGE = 'keep_resize_linear_fxy_u8'
_ENLARGED = {}


def enlarged(img):
    """``cv2.resize(img, (0, 0), fx=f, fy=f, INTER_LINEAR)`` with f = 512.0 / min(h, w), restated; computed once per image."""
    key = hashlib.sha1(img.tobytes()).hexdigest()
    if key not in _ENLARGED:
        f = 512.0 / min(img.shape[:2])
        out = F.resize_linear_fxy(img, f, f)
        out.setflags(write=False)
        _ENLARGED[key] = out
    return _ENLARGED[key]


def small_helper_class():
    import synth_facehelper as SF

    class SmallFrameHelper(SF.SynthFaceHelper):
        """``read_image`` as the reference's: a frame whose short side is below 512 is enlarged (:182-184).  The track geometry of the
        base class is laid out in the frame the helper was built for -- the ENLARGED frame."""
        reads = 0

        def read_image(self, img):
            self.reads += 1
            self.input_img, self.is_gray = img, False
            if min(img.shape[:2]) < 512:
                self.input_img = enlarged(img).copy()
    return SmallFrameHelper


class SmallRig(Rig):
    def __init__(self, net, monkeypatch, hw, faces, chunk, knob=None):
        f = 512.0 / min(hw)
        w2, h2 = F.enlarged_size(hw[0], hw[1], f, f)
        if knob is None:
            monkeypatch.delenv('KEEP_AMD_GPU_SMALL_FRAMES', raising=False)
        else:
            monkeypatch.setenv('KEEP_AMD_GPU_SMALL_FRAMES', knob)
        super().__init__(net, monkeypatch, (h2, w2), faces, chunk)
        self.hw2 = (h2, w2)
        self.helper.__class__ = small_helper_class()
        self.inverse = []                                   # per pasted frame, in order: the helper's crop -> output-frame matrices
        own = self.helper.get_inverse_affine

        def rec(*a, **kw):
            own(*a, **kw)
            self.inverse.append([np.array(M) for M in self.helper.inverse_affine_matrices])
        self.helper.get_inverse_affine = rec

    def run(self, frames, store, factor=1.0, comfy=None, clip=4):
        """``Rig.run``; ``comfy``: the float IMAGE batch the frames were made from (the node's entry) instead of a flag."""
        if store:
            self.mp.delenv('KEEP_AMD_FRAME_STORE', raising=False)
        else:
            self.mp.setenv('KEEP_AMD_FRAME_STORE', '0')
        self.mp.setenv('KEEP_AMD_STREAM_GROUPS', '3')
        for rec in (self.calls, self.backgrounds, self.batches, self.crop_shapes, self.inverse):
            rec.clear()
        self.helper.begin_sequence()
        self.helper.reads = 0
        if comfy is not None:
            out = self.proc.process_image_sequence(comfy, factor, False, False, False, max_clip_length=clip)
        else:
            out = self.proc.process_frames_u8(frames, factor, False, False, False, max_clip_length=clip)
        assert isinstance(out, torch.Tensor)
        return out, [np.asarray(f) for f in self.proc.last_restored_faces]

    def classes(self, faces_dev):
        """The ParseNet classes of uint8 BGR crops, as the paste-back takes them (:418-424)."""
        from comfyui_keep_amd.engine import hiplib as L
        x = torch.empty(faces_dev.shape, dtype=torch.float32, device=faces_dev.device)
        L.call('keep_img2tensor', faces_dev, x, faces_dev.numel() // 3)
        return self.helper.face_parse.engine.classes(x)


_VIDEO = {}


def small_video():
    """(float IMAGE batch [10,360,480,3], its uint8 BGR frames): the frames are what ``comfy_image_to_cv2`` makes of the batch, so both
    entries see the same bytes."""
    if not _VIDEO:
        from comfyui_keep_amd.modules.utils import comfy_image_to_cv2
        x = torch.rand((10, 360, 480, 3), generator=torch.Generator().manual_seed(21))
        _VIDEO['x'] = x
        _VIDEO['u8'] = [np.ascontiguousarray(comfy_image_to_cv2(x[i])) for i in range(10)]
    return _VIDEO['x'], _VIDEO['u8']


def two_lanczos(img, hw2, factor):
    """The reference's two background resizes, restated: to the original size times the factor (keep_processor.py:284-286 of the
    reference; the identity at factor 1), then to the enlarged size times the factor (face_restoration_helper.py:357-358)."""
    h, w = img.shape[:2]
    first = img if factor == 1 else RL.resize_lanczos4(img, int(w * factor), int(h * factor))
    return RL.resize_lanczos4(first, int(hw2[1] * factor), int(hw2[0] * factor))


@pytest.mark.parametrize('factor', [1.0, 2.0])
def test_small_sequence_stays_on_the_device(net, monkeypatch, factor):
    """10 frames of 360 x 480 (enlarged: 512 x 683), 2 face tracks, clips of 4, detection chunks of 4 frames (3 chunks)."""
    from comfyui_keep_amd.engine.paste import GpuPaster
    from comfyui_keep_amd.engine.resize import Lanczos4Resizer
    n, faces = 10, 2
    x, frames = small_video()
    big = [enlarged(f).copy() for f in frames]
    rig = SmallRig(net, monkeypatch, (360, 480), faces, chunk=4)
    assert rig.hw2 == (512, 683)
    H3, W3 = int(512 * factor), int(683 * factor)

    # (c) today's store path over the pre-enlarged frames (read_image leaves a 512 x 683 frame alone)
    _, plain_faces = rig.run(big, store=True, factor=factor)
    assert rig.count(ENLARGE) == 0 and rig.count(WARP_BATCH) == 3 and rig.helper.reads == n

    got, got_faces = rig.run(frames, store=True, factor=factor)
    backgrounds, batches, inverse = list(rig.backgrounds), list(rig.batches), list(rig.inverse)
    # (e) one enlargement and one warp call per chunk, no single warp, read_image for the probe alone, nothing on the host
    assert rig.count(ENLARGE) == 3 and rig.count(WARP_BATCH) == 3 and rig.count(WARP) == 0
    assert rig.helper.reads == 1 and rig.helper.detector_calls == 0
    assert rig.crop_shapes == [('Tensor', n * faces)]
    assert len(backgrounds) == n and all(isinstance(b, torch.Tensor) and b.is_cuda for b in backgrounds)
    assert len(batches) == 3 and all(isinstance(b, torch.Tensor) and b.is_cuda for b in batches)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, H3, W3, 3)
    assert rig.proc.frame_store is True and rig.proc.gpu_small_frames is True
    # (a) every detector batch is the restated enlargement of its frames
    assert [tuple(b.shape) for b in batches] == [(4, 512, 683, 3), (4, 512, 683, 3), (2, 512, 683, 3)]
    seen = torch.cat([b.cpu() for b in batches]).numpy()
    for t in range(n):
        assert np.array_equal(seen[t], big[t]), t
    # (b) every paste background is the restatement of the original at the enlarged size.  At factor 2 the numpy restatement of one
    # frame's two resizes takes a second: there every background is held to the device Lanczos resize applied twice (pinned to the
    # restatement by tests/test_gpu_resize.py), and one frame of each chunk to the restatement itself
    assert all(tuple(b.shape) == (H3, W3, 3) for b in backgrounds)
    if factor == 1.0:
        for t in range(n):
            assert np.array_equal(backgrounds[t].cpu().numpy(), two_lanczos(frames[t], rig.hw2, factor)), t
    else:
        rz = Lanczos4Resizer('cuda')
        for t in range(n):
            twice = rz.resize_u8(rz.resize_u8(frames[t], int(480 * factor), int(360 * factor)), W3, H3)
            assert torch.equal(backgrounds[t], twice), t
        for t in (0, 5, 9):
            assert np.array_equal(backgrounds[t].cpu().numpy(), two_lanczos(frames[t], rig.hw2, factor)), t
    # (c) the restored faces
    assert len(got_faces) == len(plain_faces) == n * faces and all(np.array_equal(a, b) for a, b in zip(got_faces, plain_faces))
    # (d) every output frame is the paste of its faces onto its background with the helper's inverse affines
    assert len(inverse) == n and all(len(m) == faces for m in inverse)
    paster = GpuPaster('cuda')
    for t in range(n):
        fd = torch.from_numpy(np.stack(got_faces[faces * t:faces * t + faces])).cuda()
        want = paster.paste(backgrounds[t], fd, inverse[t], rig.classes(fd), factor, False)
        assert torch.equal(got[t], want.cpu()), t
        assert (want != backgrounds[t]).any()                                          # (faces were really pasted)
    # (f) the node's float entry: the same bits after conversion
    got_f, faces_f = rig.run(frames, store=True, factor=factor, comfy=x)
    assert rig.count(ENLARGE) == 3 and rig.count(WARP_BATCH) == 3 and rig.count(WARP) == 0 and rig.helper.reads == 1
    assert all(isinstance(b, torch.Tensor) and b.is_cuda for b in rig.backgrounds + rig.batches)
    assert got_f.dtype == torch.float32 and torch.equal(got_f, got.flip(-1).float() / 255.0)
    assert all(np.array_equal(a, b) for a, b in zip(faces_f, got_faces))


def test_without_the_store_the_background_has_the_enlarged_size(net, monkeypatch):
    """KEEP_AMD_FRAME_STORE=0 on the same video: the streamed paste used to composite faces whose inverse affines live in the 512 x 683
    frame onto the 360 x 480 background.  Now it is the store path's output bit for bit, at factor 1 and 2."""
    n, faces = 10, 2
    _, frames = small_video()
    rig = SmallRig(net, monkeypatch, (360, 480), faces, chunk=4)
    for factor in (1.0, 2.0):
        H3, W3 = int(512 * factor), int(683 * factor)
        got, got_faces = rig.run(frames, store=False, factor=factor)
        print(f"factor {factor}: output {tuple(got.shape)}, backgrounds {sorted(set(tuple(b.shape) for b in rig.backgrounds))}")
        assert rig.count(ENLARGE) == 0 and rig.count(WARP) == n * faces and rig.count(WARP_BATCH) == 0
        assert rig.helper.reads == 2 * n                                               # the pre-pass and the crop loop, as before
        assert len(rig.backgrounds) == n and all(tuple(b.shape) == (H3, W3, 3) for b in rig.backgrounds)
        assert tuple(got.shape) == (n, H3, W3, 3)
        ref, ref_faces = rig.run(frames, store=True, factor=factor)
        assert rig.count(ENLARGE) == 3
        print(f"factor {factor}: {int((got != ref).sum()) if got.shape == ref.shape else 'n/a'} values differ from the store path")
        assert torch.equal(got, ref)
        assert all(np.array_equal(a, b) for a, b in zip(got_faces, ref_faces))
    # the knob off keeps that path with the store asked for: read_image changed the frames, the store ends quietly
    off = SmallRig(net, monkeypatch, (360, 480), faces, chunk=4, knob='0')
    assert off.proc.gpu_small_frames is False
    got, _ = off.run(frames, store=True, factor=2.0)
    assert off.count(ENLARGE) == 0 and off.count(WARP) == n * faces and off.helper.reads == 2 * n and torch.equal(got, ref)
    assert off.proc.frame_store is True


def test_single_small_image_keeps_the_gpu_paste(net, monkeypatch):
    """A 300 x 400 image through ``process_image``: ``read_image`` enlarges it to 512 x 683, the background fails the size test of the GPU
    paste alone and is brought there on the device.  (The synthetic helper has no paste of its own: it raises.)  Equal to frame 0 of the
    duplicated one-face clip, pasted directly onto the restated background."""
    from comfyui_keep_amd.engine.paste import GpuPaster, crop_faces
    rig = SmallRig(net, monkeypatch, (300, 400), 1, chunk=4)
    assert rig.hw2 == (512, 683)
    img = np.random.default_rng(12).integers(0, 256, (300, 400, 3), dtype=np.uint8)
    rig.helper.begin_sequence()
    out = rig.proc.process_image(img, 1.0, False, False, False)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (512, 683, 3)
    assert rig.count('keep_resize_lanczos4_u8') == 1 and len(rig.backgrounds) == 1
    bg = rig.backgrounds[0]
    assert isinstance(bg, torch.Tensor) and bg.is_cuda and np.array_equal(bg.cpu().numpy(), RL.resize_lanczos4(img, 683, 512))
    assert len(rig.helper.affine_matrices) == 1 and len(rig.inverse) == 1
    crop = crop_faces(enlarged(img).copy(), list(rig.helper.affine_matrices), (512, 512), 'cuda')[0].cpu().numpy()
    restored = net.run_clips_u8([[crop, crop]])[0][0].numpy()
    assert np.array_equal(restored, np.asarray(rig.proc.last_restored_faces[0]))
    fd = torch.from_numpy(restored[None].copy()).cuda()
    want = GpuPaster('cuda').paste(bg, fd, rig.inverse[0], rig.classes(fd), 1.0, False).cpu().numpy()
    assert np.array_equal(out, want) and (want != bg.cpu().numpy()).any()
