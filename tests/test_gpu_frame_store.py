"""GPU suite (-m gpu): a detected sequence whose frames stay on the device from the detection pre-pass to the paste-back
(modules/keep_processor.py: ``_FrameStore``, ``_stored_sequence``; KEEP_AMD_FRAME_STORE) against the present path
(KEEP_AMD_FRAME_STORE=0: every frame uploaded for the detector, again per frame for the crop warp, again for the paste) -- the same
output BIT FOR BIT, through the product's own entry points over tools/synth_facehelper.py like tests/test_gpu_paste.py, with the
library calls of both paths counted."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

WARP, WARP_BATCH, AREA = 'keep_warp_affine_u8', 'keep_warp_affine_batch_u8', 'keep_resize_area_u8'


@pytest.fixture(scope='module')
def net(synth_weights):
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth_weights, strict=True)
    net.to('cuda').eval()
    return net


def video(n, h, w, seed=5):
    return [f for f in np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)]


class Rig:
    """One processor over the synthetic helper, with the library calls, the paste backgrounds and the detector batches recorded."""

    def __init__(self, net, monkeypatch, hw, faces, chunk):
        import synth_facehelper as SF
        from comfyui_keep_amd.engine import hiplib as L
        from comfyui_keep_amd.engine.paste import GpuPaster
        self.mp = monkeypatch
        self.proc, self.helper = SF.make_processor(net, hw, faces)
        self.proc.keep_restored_faces = True
        self.proc.gpu_resize = self.proc.gpu_detect_resize = True
        self.det = self.helper.face_detector
        self.det.engine.max_frames = chunk
        self.calls, self.backgrounds, self.batches, self.crop_shapes = [], [], [], []
        real_call = L.call
        monkeypatch.setattr(L, 'call', lambda name, *a: (self.calls.append(name), real_call(name, *a))[1])
        real_paste = GpuPaster.paste

        def paste(this, frame_u8, *a, **kw):
            self.backgrounds.append(frame_u8)
            return real_paste(this, frame_u8, *a, **kw)
        monkeypatch.setattr(GpuPaster, 'paste', paste)
        real_batch = self.det.detect_batch

        def detect_batch(x, *a, **kw):
            self.batches.append(x)
            return real_batch(x, *a, **kw)
        monkeypatch.setattr(self.det, 'detect_batch', detect_batch)
        real_stream = self.proc._restore_and_paste_streamed

        def streamed(frames_bgr, crops, *a, **kw):
            self.crop_shapes.append((type(crops).__name__, len(crops)))
            return real_stream(frames_bgr, crops, *a, **kw)
        monkeypatch.setattr(self.proc, '_restore_and_paste_streamed', streamed)

    def run(self, frames, store, factor=1.0, comfy=False, clip=4):
        if store:
            self.mp.delenv('KEEP_AMD_FRAME_STORE', raising=False)
        else:
            self.mp.setenv('KEEP_AMD_FRAME_STORE', '0')
        self.mp.setenv('KEEP_AMD_STREAM_GROUPS', '3')
        for rec in (self.calls, self.backgrounds, self.batches, self.crop_shapes):
            rec.clear()
        self.helper.begin_sequence()
        if comfy:
            x = torch.from_numpy(np.stack(frames)[..., ::-1].copy()).float() / 255.0
            out = self.proc.process_image_sequence(x, factor, False, False, False, max_clip_length=clip)
        else:
            out = self.proc.process_frames_u8(frames, factor, False, False, False, max_clip_length=clip)
        assert isinstance(out, torch.Tensor)                       # the streamed paste took the sequence, store or not
        return out, [np.asarray(f) for f in self.proc.last_restored_faces]

    def count(self, name):
        return self.calls.count(name)


def test_store_equals_the_present_path(net, monkeypatch):
    """10 frames of 360 x 480, 2 face tracks, clips of 4 in >= 2 batch groups, detection chunks of 4 frames (3 chunks).  No detector
    resize at this size: the stored chunk is the detector batch itself."""
    n, faces = 10, 2
    rig = Rig(net, monkeypatch, (360, 480), faces, chunk=4)
    frames = video(n, 360, 480)
    ref, ref_faces = rig.run(frames, store=False)
    assert rig.count(WARP) == n * faces and rig.count(WARP_BATCH) == 0
    assert len(rig.backgrounds) == n and all(isinstance(b, np.ndarray) for b in rig.backgrounds)
    assert rig.helper.detector_calls == 0
    got, got_faces = rig.run(frames, store=True)
    assert rig.count(WARP) == 0 and rig.count(WARP_BATCH) == 3                     # one call per chunk
    assert len(rig.backgrounds) == n and all(isinstance(b, torch.Tensor) and b.is_cuda for b in rig.backgrounds)
    assert len(rig.batches) == 3 and all(isinstance(b, torch.Tensor) and b.is_cuda for b in rig.batches)
    assert [tuple(b.shape) for b in rig.batches] == [(4, 360, 480, 3), (4, 360, 480, 3), (2, 360, 480, 3)]
    assert rig.crop_shapes == [('Tensor', n * faces)]
    assert rig.helper.detector_calls == 0
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 360, 480, 3) and torch.equal(got, ref)
    assert len(got_faces) == len(ref_faces) == n * faces and all(np.array_equal(a, b) for a, b in zip(got_faces, ref_faces))
    assert (got != torch.from_numpy(np.stack(frames))).any()                       # (faces were really pasted)
    assert rig.proc.frame_store is True
    # the node's float entry: the frames come out of the pinned conversion buffer
    ref_f, ref_faces_f = rig.run(frames, store=False, comfy=True)
    assert rig.count(WARP) == n * faces and rig.count(WARP_BATCH) == 0
    got_f, got_faces_f = rig.run(frames, store=True, comfy=True)
    assert rig.count(WARP) == 0 and rig.count(WARP_BATCH) == 3
    assert all(isinstance(b, torch.Tensor) and b.is_cuda for b in rig.backgrounds + rig.batches)
    assert got_f.dtype == torch.float32 and torch.equal(got_f, ref_f)
    assert all(np.array_equal(a, b) for a, b in zip(got_faces_f, ref_faces_f))
    assert rig.helper.detector_calls == 0


def test_detector_resize_reads_the_store(net, monkeypatch):
    """4 frames of 672 x 896 with a helper that brings no resize of its own: the detector input is 640 x 853, resized on the device from
    the stored chunk -- one keep_resize_area_u8 launch per chunk of 2 frames, no second copy of the frames."""
    from comfyui_keep_amd.engine.resize import area_geometry_refused
    assert not area_geometry_refused(672, 896, 640, 853)
    rig = Rig(net, monkeypatch, (672, 896), 1, chunk=2)
    rig.helper.resize_for_detector = None
    frames = video(4, 672, 896, seed=6)
    ref, _ = rig.run(frames, store=False)
    assert rig.count(AREA) == 2 and rig.count(WARP) == 4
    off_batches = [b.cpu() for b in rig.batches]
    got, _ = rig.run(frames, store=True)
    assert rig.count(AREA) == 2 and rig.count(WARP) == 0 and rig.count(WARP_BATCH) == 2
    assert [tuple(b.shape) for b in rig.batches] == [(2, 640, 853, 3)] * 2 and all(b.is_cuda for b in rig.batches)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(rig.batches, off_batches))   # the detector saw the same pixels
    assert all(isinstance(b, torch.Tensor) and b.is_cuda and tuple(b.shape) == (672, 896, 3) for b in rig.backgrounds)
    assert torch.equal(got, ref) and rig.proc.gpu_detect_resize is True and rig.helper.detector_calls == 0


def test_varying_faces_and_a_frame_without_faces(net, monkeypatch):
    """Track 1 is missing on frames 0 - 2 and frame 5 has no face at all (the real smoother interpolates every gap, so a wrapper blanks
    them): 10 * 2 - 3 - 2 = 15 crops, frame 5 comes back as it went in, emitted from the store."""
    from comfyui_keep_amd.modules import keep_processor as KP
    real = KP.smooth_tracked_faces

    def blanked(raw):
        tracks = {k: np.array(v, np.float64, copy=True) for k, v in real(raw).items()}
        keys = sorted(tracks)
        assert len(keys) == 2
        tracks[keys[1]][0:3] = np.nan
        for k in keys:
            tracks[k][5] = np.nan
        return tracks
    monkeypatch.setattr(KP, 'smooth_tracked_faces', blanked)
    rig = Rig(net, monkeypatch, (360, 480), 2, chunk=4)
    frames = video(10, 360, 480, seed=7)
    ref, ref_faces = rig.run(frames, store=False)
    assert rig.count(WARP) == 15 and len(rig.backgrounds) == 9
    got, got_faces = rig.run(frames, store=True)
    assert rig.crop_shapes == [('Tensor', 15)] and rig.count(WARP) == 0 and rig.count(WARP_BATCH) == 3
    assert len(rig.backgrounds) == 9 and all(b.is_cuda for b in rig.backgrounds)
    assert torch.equal(got[5], torch.from_numpy(frames[5]))
    assert torch.equal(got, ref) and (got[4] != torch.from_numpy(frames[4])).any()
    assert len(got_faces) == 15 and all(np.array_equal(a, b) for a, b in zip(got_faces, ref_faces))


def test_factor_2_background_is_resized_from_the_store(net, monkeypatch):
    rig = Rig(net, monkeypatch, (360, 480), 2, chunk=4)
    frames = video(5, 360, 480, seed=8)
    ref, _ = rig.run(frames, store=False, factor=2.0)
    assert rig.count('keep_resize_lanczos4_u8') == 5
    got, _ = rig.run(frames, store=True, factor=2.0)
    assert rig.count('keep_resize_lanczos4_u8') == 5 and rig.count(WARP) == 0 and rig.count(WARP_BATCH) == 2
    assert all(b.is_cuda and tuple(b.shape) == (720, 960, 3) for b in rig.backgrounds)
    assert tuple(got.shape) == (5, 720, 960, 3) and torch.equal(got, ref)


def test_cap_mixed_sizes_and_failure_keep_the_present_path(net, monkeypatch, caplog):
    from comfyui_keep_amd.engine import paste
    rig = Rig(net, monkeypatch, (360, 480), 2, chunk=4)
    frames = video(5, 360, 480, seed=9)
    ref, _ = rig.run(frames, store=False)
    # over the cap (100 kB): per-face launches, the same output
    monkeypatch.setenv('KEEP_AMD_FRAME_STORE_GB', '0.0001')
    got, _ = rig.run(frames, store=True)
    assert rig.count(WARP) == 10 and rig.count(WARP_BATCH) == 0 and torch.equal(got, ref)
    assert all(isinstance(b, np.ndarray) for b in rig.backgrounds)
    monkeypatch.delenv('KEEP_AMD_FRAME_STORE_GB')
    # one frame of another size is outside the streamed paste as well: the per-frame path, one launch per face, knob on or off
    mixed = frames[:3] + video(1, 368, 480, seed=11)
    # (on the per-frame path the helper still holds the LAST frame it read, so ``_gpu_paste_applies`` hands every frame of another size to
    # the helper's own paste, which the synthetic helper does not have: a stand-in that returns the background, as in tests/test_gpu_paste.py)
    monkeypatch.setattr(rig.helper, 'paste_faces_to_input_image', lambda upsample_img=None, **kw: upsample_img)

    def run_mixed(store):
        if store:
            monkeypatch.delenv('KEEP_AMD_FRAME_STORE', raising=False)
        else:
            monkeypatch.setenv('KEEP_AMD_FRAME_STORE', '0')
        rig.calls.clear()
        rig.backgrounds.clear()
        rig.helper.begin_sequence()
        return rig.proc.process_frames_u8(mixed, 1.0, False, False, False, max_clip_length=4)
    ref_m = run_mixed(False)
    got_m = run_mixed(True)
    assert rig.count(WARP) == 8 and rig.count(WARP_BATCH) == 0
    assert len(rig.backgrounds) == 1 and isinstance(rig.backgrounds[0], np.ndarray) and rig.backgrounds[0].shape == (368, 480, 3)
    assert isinstance(got_m, list) and len(got_m) == 4 and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(got_m, ref_m))
    assert rig.proc.frame_store is True
    # the batched warp raises before anything was restored: one warning, the store off from here on, the same output
    def boom(*a, **kw):
        raise RuntimeError('injected')
    monkeypatch.setattr(paste, 'crop_faces_batch', boom)
    with caplog.at_level(logging.WARNING, logger='ComfyUI-KEEP'):
        got, _ = rig.run(frames, store=True)
    warned = [r for r in caplog.records if 'injected' in r.getMessage()]
    assert len(warned) == 1 and rig.proc.frame_store is False
    assert rig.count(WARP) == 10 and torch.equal(got, ref)
