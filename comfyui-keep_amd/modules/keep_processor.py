"""Frame / clip driver -- drop-in for reference ``modules/keep_processor.py:117-307``.

Hot loop #1 of the path: crops of all frames are stacked frame-major
(faces of one frame adjacent), cut into chunks of ``max_clip_length`` and every chunk is one
independent ``keep_net`` clip (keep_processor.py:256-270).  Behaviour kept bug-compatible:
  * multi-face sequences interleave faces inside a clip (P1);
  * a chunk of length 1 is duplicated to T=2 and frame 0 kept (keep_processor.py:266-268, 173-175);
  * with ``has_aligned_frames`` the restored faces are computed and then NOT used: the output
    is the resized input (keep_processor.py:289-291) -- see ``last_restored_faces`` below;
  * ComfyUI progress: N + N + N ticks, then one tick per frame that had faces (KP:200-304).
Detection / tracking / alignment / paste-back stay with the reference's ``FaceRestoreHelper``
(out of scope, unchanged); tracking + smoothing (KP:33-115, 216-231) are restated in
``face_tracks.py`` because they live in the reference's own glue file.

What this build adds: independent clips are handed to the engine in one call
(``keep_net.run_clips_u8``) so it can batch equal-length clips per GPU (bounded by free HBM) and,
when a torch.distributed group or the worker pool (``KEEP_AMD_GPUS``, engine/pool.py) is up, shard them across
GPUs.  Clips share no state and the kernel plans are batch-invariant (tiles / split-K follow the per-image geometry,
DESIGN.md section 6), so the result equals the sequential one-clip-at-a-time loop BIT FOR BIT
(tests/test_gpu_net.py::test_config3_config4_clip_mixes_equal_sequential).
The paste-back compositing can run on the GPU (``KEEP_AMD_GPU_PASTE``, ``_paste`` below).

Round 5 -- the sequence path STREAMS steps 3 and 4 (``_restore_and_paste_streamed``): with the engine's net, its ParseNet and the
GPU paste available, crops that were warped on the GPU stay there, the clip loop hands every finished batch group over on the
device (``run_clips_u8(sink=...)``), ParseNet runs on batches of up to 32 faces ACROSS frames (the reference: one face per call,
face_restoration_helper.py:418-424), and the frames whose faces are all restored are composited and downloaded on a second HIP
stream while the next group is being restored.  Same arithmetic, same order per frame: the output equals the per-frame path bit
for bit (tests/test_gpu_paste.py::test_streamed_sequence_equals_the_per_frame_path); every other configuration keeps that path.

Aligned inputs (``has_aligned``): a frame that is not 512 x 512 is brought there by the INTER_LINEAR resize on the device
(``_aligned_face``, KEEP_AMD_GPU_ALIGNED_RESIZE), and an aligned sequence stays on the device from upload to output
(``_aligned_streamed``), equal to the per-frame path bit for bit (tests/test_gpu_aligned.py).

Detected sequences: where the streamed paste applies, every frame is uploaded ONCE -- the detection pre-pass copies each chunk into a
device tensor that stays (``_FrameStore``): the detector resize reads it (or it is the detector batch), one ``keep_warp_affine_batch_u8``
call per chunk warps its faces into the sequence's crop tensor, whose views are the clips, and the paste-back takes its backgrounds
from it (``_stored_sequence``; KEEP_AMD_FRAME_STORE=0 keeps the three uploads per frame, KEEP_AMD_FRAME_STORE_GB caps the store).  Equal
to that path bit for bit (tests/test_gpu_frame_store.py).

Small frames: a helper whose ``read_image`` enlarges every frame with a short side below 512 (face_restoration_helper.py:182-184) used to end
the store.  Where the first frame's ``read_image`` shows that enlargement, the store keeps each chunk twice -- the original frames and
their enlargement by one ``keep_resize_linear_fxy_u8`` launch, which is the detector batch and the source of the crop warp -- and the
paste-back resizes the originals to the enlarged size (KEEP_AMD_GPU_SMALL_FRAMES; tests/test_gpu_small_frames.py).  Without the store the
streamed paste brings each background to the size ``read_image`` made before it composites.

Track clips (``KEEP_AMD_TRACK_CLIPS``, off by default): the repaired form of P1 and P3 -- every clip holds consecutive frames of one face
track (``clip_plan.py``), every face of a single image is a clip of its own.  Crop numbering and the paste order stay; the frame store lays
its crop tensor out by clip (``keep_warp_affine_batch_scatter_u8``) so the clips remain views.  With the knob off nothing plans, permutes or
scatters.  No reference to compare with: each face equals its track restored on its own, bit for bit (tests/test_gpu_track_clips.py).

Carried clips (``KEEP_AMD_TRACK_CARRY``, off by default, implies track clips): a clip that continues a run of its track starts from the state
its predecessor left instead of from nothing (``clip_plan.plan_track_chains`` names the predecessor, ``run_clips_u8(after=...)`` hands the
state over), on every path a sequence takes; an aligned sequence is one track.  One process only (tests/test_gpu_track_carry.py).

Scene cuts (``KEEP_AMD_SCENE_CUTS``, off by default, implies track clips): consecutive frames whose signatures (``scene_cuts.py``: a grid of
luma histograms; ``keep_frame_signature_u8`` on the chunks the frame store holds, the host restatement elsewhere -- the same integers) are
at least ``scene_cut_threshold`` apart are a hard cut: every scene is tracked and smoothed on its own, no clip spans a cut and no state
is carried across one.  A video of scenes A then B equals A and B processed as two videos, bit for bit (tests/test_gpu_scene_cuts.py).

Track lifetimes (``KEEP_AMD_TRACK_LIFETIMES``, off by default, implies track clips): the reference's smoothing holds a track's end values
over the whole video, so every track has a face on every frame, and one detector miss ends a track and starts a duplicate.  With the knob
the raw tracks are stitched over gaps of at most ``track_max_gap`` frames and a track lives from its first to its last detection
(``face_tracks.py``); outside it nothing is cropped, restored or pasted.  A lifetime equals its frames processed as a video of their own,
bit for bit (tests/test_gpu_track_lifetimes.py).  ``track_fade`` ramps the paste weight at a lifetime's ends (``keep_paste_face_w``).

Alias-free paste-back (``KEEP_AMD_PASTE_AA``, off by default): the paste-back takes one bilinear tap of the restored crop per frame pixel,
which aliases wherever the face is shrunk on its way back -- and real faces are, 2 to 5.5 times.  With the knob the GPU paste area-samples
every shrunk face (``engine/paste.py``: ``aa_factor``, ``keep_paste_face_aa``); a face that is not shrunk takes today's calls.  The knob is
one keyword at the three ``paster.paste`` call sites; the network, ParseNet and ``last_restored_faces`` never see it
(tests/test_gpu_paste_aa_processor.py).  No parity mode.

One form of each thing: the clips of a crop list are lists of crop indices everywhere -- the flat cut is the plan whose clip c is
``range(start, end)`` of span c (``_restore_crops_u8``, ``_restore_clips``, ``_restore_and_paste_streamed``); every device path that stands
in for a cv2 call is decided by ``_gate`` from a row of ``opencv_checks.GATES``; both streamed paths write their output through
``_HostOutput``.  The self-checks against cv2 live in ``opencv_checks.py``, the frame containers (``_ConvertedFrames``, ``_FrameStore``) in
``frames.py``; their names are importable from here as before.
"""
import logging
import os

import numpy as np
import torch
from tqdm import tqdm

from . import opencv_checks
from .frames import (FRAME_STORE_DEFAULT_GB, _ConvertedFrames, _FrameStore, cuda_device, frame_store_plan,  # noqa: F401  (the containers
                     frames_from_comfy, uniform_u8_frames)                                                 # are read from here too)
from .opencv_checks import (opencv_agrees_with_gpu_aligned_resize, opencv_agrees_with_gpu_detect_resize,  # noqa: F401  (read from here by
                            opencv_agrees_with_gpu_paste, opencv_agrees_with_gpu_resize,                  # tests and tools; the gate itself
                            opencv_agrees_with_gpu_small_frame_resize)                                    # asks ``opencv_checks``)
from .utils import comfy_image_to_cv2, crops_to_net_input, cv2_to_comfy_image, net_output_to_bgr_u8
from .face_tracks import fade_weights, smooth_center_face, smooth_tracked_faces

log = logging.getLogger('ComfyUI-KEEP')

try:  # ComfyUI runtime
    from comfy.utils import ProgressBar, tiled_scale
except ModuleNotFoundError:  # engine-only use outside ComfyUI
    tiled_scale = None

    class ProgressBar:  # minimal stand-in with the same calls
        def __init__(self, total):
            self.total, self.current = total, 0

        def update(self, n):
            self.current += n


def _cv2():
    import cv2
    return cv2


def _resize(img, w, h, interp_name):
    if img.shape[0] == h and img.shape[1] == w:
        return img
    cv2 = _cv2()
    return cv2.resize(img, (w, h), interpolation=getattr(cv2, interp_name))


def _is_gray(img, threshold=10):
    """wm_facelib/utils/misc.py:146-160: mean variance of channel differences <= threshold."""
    if img.ndim == 2:
        return True
    c = img.astype(np.int16)
    d = ((c[..., 0] - c[..., 1]).var() + (c[..., 1] - c[..., 2]).var() + (c[..., 2] - c[..., 0]).var()) / 3.0
    return bool(d <= threshold)


def small_frame_factor(h, w):
    """``f`` of ``read_image``'s enlargement (face_restoration_helper.py:182-184) for an [h,w] frame, or None where it does not enlarge."""
    return 512.0 / min(h, w) if 0 < min(h, w) < 512 else None


def _host(img):
    """A background / face that leaves the device path (the helper's own paste, a frame returned as it is): a host array."""
    return img.cpu().numpy() if isinstance(img, torch.Tensor) else img


def _env_number(name, default, cast):
    """The environment's ``name`` as ``cast`` (int / float); unset, empty or not a number: ``default``."""
    try:
        return cast(os.environ.get(name, '') or default)
    except ValueError:
        return default


def _env_tristate(name):
    """The environment's ``name``: '1' True, '0' False, anything else None (auto: ``KEEPFaceProcessor._gate`` decides)."""
    return {'1': True, '0': False}.get(os.environ.get(name))


def _sink_streaming(net):
    """What both streamed paths ask first: ``KEEP_AMD_STREAM_PASTE`` is not 0, the net is the engine's (``run_clips_u8`` with ``sink``),
    and the call is not inside a torch.distributed job."""
    if os.environ.get('KEEP_AMD_STREAM_PASTE', '1') == '0' or not getattr(net, 'supports_sink', False):
        return False
    return not (torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1)


class _HostOutput:
    """The output tensor of a streamed path, [n,H',W',3] in host memory: uint8 BGR (``as_u8``) or ComfyUI's float RGB.  Allocated by the
    first ``emit``, which knows the frame size."""

    def __init__(self, n, as_u8, device):
        self.n, self.as_u8, self.device, self.out = n, as_u8, device, None

    def emit(self, f0, frames_dev):
        """finished frames f0 .. (uint8 BGR [m,H',W',3] on the device) -> the output tensor, queued on the current stream"""
        if self.out is None:
            shape, dtype = (self.n,) + tuple(frames_dev.shape[1:]), torch.uint8 if self.as_u8 else torch.float32
            try:
                self.out = torch.empty(shape, dtype=dtype, pin_memory=True)
            except RuntimeError:                                  # more than the host will pin: pageable memory, slower copies
                self.out = torch.empty(shape, dtype=dtype)
        dst = self.out[f0:f0 + frames_dev.shape[0]]
        if self.as_u8:
            dst.copy_(frames_dev, non_blocking=True)
        else:                                                      # cv2_to_comfy_image on the device (keep_bgr_u8_to_comfy: one IEEE division)
            from ..engine import hiplib as L
            ff = torch.empty(frames_dev.shape, dtype=torch.float32, device=self.device)
            L.call('keep_bgr_u8_to_comfy', frames_dev.contiguous(), ff, frames_dev.numel() // 3)
            dst.copy_(ff, non_blocking=True)


class _ReplayDetector:
    """Stands in for ``face_detector`` while the helper post-processes ONE frame of a batched detection pass: returns the
    stored ``detect_faces`` result of that frame."""

    def __init__(self, result):
        self.result = result

    def detect_faces(self, image, conf_threshold=0.8, *args, **kwargs):
        return self.result


class _DeviceFaces:
    """``last_restored_faces`` of the streamed path: the restored crops stay where they were produced (the GPU, or host memory for a
    pool worker's) and are fetched on access -- nothing downloads 236 MB per 300 crops for a list only tests and tools read."""

    def __init__(self, items):
        self._items = list(items)

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self._items)))]
        t = self._items[i]
        return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))

    def __iter__(self):
        return (self[i] for i in range(len(self._items)))


_EMITTED = object()   # placeholder of a restored crop whose frame has been composited (streamed path)


def split_clips(num_faces: int, max_clip_length: int):
    """[(start, end)] chunk boundaries of the flat crop list (keep_processor.py:263-264)."""
    return [(s, min(s + max_clip_length, num_faces)) for s in range(0, num_faces, max_clip_length)]


class KEEPFaceProcessor:
    def __init__(self, model_pack):
        self.keep_net = model_pack.keep_net
        self.face_helper = model_pack.face_helper
        self.bg_upscale_model = model_pack.bg_upscale_model
        self.face_upscale_model = model_pack.face_upscale_model
        self.device = model_pack.device
        self.model_type_str = model_pack.model_type_str
        # restored 512x512 faces of the last call, uint8 BGR (the reference discards them on the
        # aligned-sequence path; exposed so callers / tests can read what the net produced)
        self.last_restored_faces = []
        # streamed sequence path: keep the restored crops (on the GPU) in ``last_restored_faces`` after the call -- off by default
        self.keep_restored_faces = os.environ.get('KEEP_AMD_KEEP_RESTORED', '0') == '1'
        # reference quirk P2: `KEEP Image Sequence` with has_aligned=True restores every frame
        # and then returns the *input* frames.  Default: bug-compatible.  KEEP_AMD_RETURN_RESTORED_ALIGNED=1 (or setting
        # the attribute) returns the restored faces instead.
        self.return_restored_aligned = os.environ.get('KEEP_AMD_RETURN_RESTORED_ALIGNED', '0') == '1'
        # reference quirks P1 / P3: with several faces in the picture the flat frame-major crop list is cut into clips, so a clip
        # interleaves identities (A0 B0 C0 A1 ...), and the single-image node makes ONE clip of all its faces.  Default: bug-compatible.
        # KEEP_AMD_TRACK_CLIPS=1 (or setting the attribute): every clip holds consecutive frames of one track (``clip_plan.py``), every
        # face of a single image is a clip of its own.  With one face per frame the clips are the default's.
        self.track_clips = os.environ.get('KEEP_AMD_TRACK_CLIPS', '0') == '1'
        # ``max_clip_length`` bounds memory, yet every clip starts the net's recurrence from nothing: frame 0 of a clip is decoded without
        # warp, Kalman update or CFA.  KEEP_AMD_TRACK_CARRY=1 (or setting the attribute; implies track clips): a clip that continues a track's
        # run starts from the state its predecessor left (``plan_track_chains``, ``KeepNet.run_clips_u8(after=...)``), so the cut into
        # clips no longer shows in a track's pixels.  No parity mode -- the reference never does this.  One process only.
        self.track_carry = os.environ.get('KEEP_AMD_TRACK_CARRY', '0') == '1'
        # tracking, smoothing and the carried state all assume that consecutive frames show one scene; edited video has hard cuts.
        # KEEP_AMD_SCENE_CUTS=1 (or setting the attribute; implies track clips): frames whose signatures (``scene_cuts.py``) are at least
        # ``scene_cut_threshold`` apart (KEEP_AMD_SCENE_CUT_THRESHOLD, default 0.4: a setting, not a measured optimum) open a new scene,
        # every scene is tracked and smoothed on its own, no clip spans a cut and nothing is carried across one.  A false cut costs one
        # state reset, which every clip boundary causes by default anyway; a missed cut leaves today's behaviour.  After a call with the
        # knob on ``last_scene_cuts`` (list of int) and ``last_scene_distances`` (float [n - 1]) say what was found.
        self.scene_cuts = os.environ.get('KEEP_AMD_SCENE_CUTS', '0') == '1'
        self.scene_cut_threshold = _env_number('KEEP_AMD_SCENE_CUT_THRESHOLD', 0.4, float)
        # the reference's gap interpolation holds a track's end values (np.interp), so a face seen on 10 of 300 frames is cropped, restored
        # and pasted on all 300, and a track that misses one detection dies and is doubled by the new track of the same person.
        # KEEP_AMD_TRACK_LIFETIMES=1 (or setting the attribute; implies track clips): raw tracks are stitched over gaps of at most
        # ``track_max_gap`` frames (KEEP_AMD_TRACK_MAX_GAP, default 10: a setting, not a measured optimum) and a track lives from its first to
        # its last detection (``face_tracks.py``).  ``track_fade`` (KEEP_AMD_TRACK_FADE, default 0 frames): the paste weight ramps over that
        # many frames at an end of a lifetime that is not an end of the video or of a scene.  No parity mode and no re-identification
        # tracker.  A single image and an aligned sequence ignore the knob.  After a call with the knob on ``last_track_lifetimes`` lists
        # (key, first_frame, last_frame, n_detections).
        self.track_lifetimes = os.environ.get('KEEP_AMD_TRACK_LIFETIMES', '0') == '1'
        self.track_max_gap = max(0, _env_number('KEEP_AMD_TRACK_MAX_GAP', 10, int))
        self.track_fade = max(0, _env_number('KEEP_AMD_TRACK_FADE', 0, int))
        # the paste-back takes ONE bilinear tap of the restored 512 x 512 crop per frame pixel (cv2.warpAffine INTER_LINEAR, restated bit for
        # bit); a face of 90 .. 250 px is that crop shrunk 2 .. 5.5 times, so the tap aliases and the pattern crawls from frame to frame.
        # KEEP_AMD_PASTE_AA=1 (or setting the attribute): the GPU paste area-samples every shrunk face -- N x N sub-samples per frame pixel,
        # N from the face's own scale (``engine/paste.py``: ``aa_factor``, ``keep_paste_face_aa``); a face that is not shrunk (N = 1) takes
        # today's calls.  No parity mode, and nothing below a scale of 1/8.  Where the helper's own paste takes a frame the knob is ignored
        # with one logged warning.  After a call with the knob on ``last_paste_aa`` is {N: faces pasted with it}.
        self.paste_aa = os.environ.get('KEEP_AMD_PASTE_AA', '0') == '1'
        # paste-back compositing on the GPU (engine/paste.py).  Opt-in: its arithmetic restates OpenCV's and
        # could not be checked against cv2 itself in the build image.
        # KEEP_AMD_GPU_PASTE: '1' on, '0' off; unset = 'auto': the first paste runs ``opencv_agrees_with_gpu_paste`` -- the HIP
        # path against cv2 itself on a synthetic 1080p / 3-face frame, bit for bit -- and switches the GPU path on only if that
        # holds on this installation (cv2 is a hard dependency of the reference helper, so it exists wherever this code pastes).
        self.gpu_paste = _env_tristate('KEEP_AMD_GPU_PASTE')
        self._gpu_paste_forced = os.environ.get('KEEP_AMD_GPU_PASTE') == '1'        # the erosion-mask branch (use_parse=False) is not part of the cv2 self-check
        self._paster = None
        self._resizers = {}             # ``_resizer``: one per class of engine/resize.py, built on first use
        # final_upscale_factor != 1: the INTER_LANCZOS4 resize of the background (and of aligned outputs) on the device
        # (engine/resize.py).  KEEP_AMD_GPU_RESIZE: '1' on, '0' off (cv2.resize on the host); unset = auto: with cv2 the first resize
        # runs ``opencv_agrees_with_gpu_resize`` and the device path is used only if it is bit-equal to cv2; without cv2 the device
        # path is the only one there is.
        self.gpu_resize = _env_tristate('KEEP_AMD_GPU_RESIZE')
        # the INTER_AREA resize of the detector inputs (face_restoration_helper.py:206-216) on the device (engine/resize.py:AreaResizer;
        # ``_prep_detect_chunk``).  KEEP_AMD_GPU_DETECT_RESIZE: '1' on, '0' off; unset = auto, decided like KEEP_AMD_GPU_RESIZE: with cv2
        # by ``opencv_agrees_with_gpu_detect_resize`` once per processor, without cv2 the device path.
        self.gpu_detect_resize = _env_tristate('KEEP_AMD_GPU_DETECT_RESIZE')
        # has_aligned: the INTER_LINEAR resize of a frame that is not 512 x 512 already (keep_processor.py:158,250 of the reference) on the
        # device (engine/resize.py:LinearResizer; ``_aligned_face``, ``_aligned_streamed``).  KEEP_AMD_GPU_ALIGNED_RESIZE: '1' on, '0' off;
        # unset = auto, decided like the two above: with cv2 by ``opencv_agrees_with_gpu_aligned_resize`` once per processor, without cv2
        # the device path.
        self.gpu_aligned_resize = _env_tristate('KEEP_AMD_GPU_ALIGNED_RESIZE')
        # read_image's enlargement of frames whose short side is below 512 (face_restoration_helper.py:182-184) on the device
        # (LinearResizer.enlarge_u8; ``_small_frames_probe``): such a sequence keeps its frame store.  KEEP_AMD_GPU_SMALL_FRAMES: '1' on,
        # '0' off; unset = auto, decided like the three above: with cv2 by ``opencv_agrees_with_gpu_small_frame_resize`` once per
        # processor, without cv2 the device path.
        self.gpu_small_frames = _env_tristate('KEEP_AMD_GPU_SMALL_FRAMES')
        # the detected-face sequence path keeps every frame on the device from the detection pre-pass to the paste-back (``_FrameStore``,
        # ``_stored_sequence``) where the streamed paste applies.  KEEP_AMD_FRAME_STORE=0 (read per call): off; KEEP_AMD_FRAME_STORE_GB: the cap.  A failure
        # while filling or warping turns it off for this processor (``frame_store = False``).
        self.frame_store = True
        self.detect_resize = 640        # the sequence pre-pass's ``resize`` of get_face_landmarks_5 (keep_processor.py:207-213 of the reference)

    # ------------------------------------------------------------------ net invocation
    def _restore_clips(self, crops_tensor, members):
        """crops_tensor [1,N,3,512,512] on device, the clips as crop indices (a range or a list per clip; every crop in exactly one)
        -> [N,3,512,512] restored (fp32, unclamped), in crop order."""
        clips = []
        for m in members:
            clip = crops_tensor[:, m.start:m.stop] if isinstance(m, range) else crops_tensor[:, m]    # (a span of the flat cut: a view)
            if len(m) == 1 and not getattr(self.keep_net, 'supports_single_frame', False):
                clip = torch.cat([clip, clip], dim=1)    # the reference net needs T>=2 (KP:173-178); frame 0 is kept
            clips.append(clip)
        run_clips = getattr(self.keep_net, 'run_clips', None)
        if run_clips is not None:                        # engine: batch / shard independent clips
            outs = run_clips(clips, need_upscale=False)
        else:
            outs = [self.keep_net(c, need_upscale=False) for c in tqdm(clips, desc="Restoring faces with KEEP")]
        restored = [None] * crops_tensor.shape[1]
        for m, o in zip(members, outs):
            for k, i in enumerate(m):
                restored[i] = o[0, k]
        return torch.stack(restored)

    def _restore_crops_u8(self, crops, max_clip_length, members=None, after=None):
        """list of uint8 BGR [512,512,3] crops -> list of restored uint8 BGR crops (same order).

        The clips are the cut of the flat list into chunks of ``max_clip_length`` (keep_processor.py:263-270); when the net offers
        ``run_clips_u8`` the uint8<->fp32 conversions of keep_processor.py:258-259,272-273 run on the GPU and only uint8 crosses PCIe,
        otherwise the host converters are used (reference behaviour).

        ``members`` (track clips): the clips as lists of crop indices (``plan_track_clips``) instead of that cut -- which is the plan whose
        clip c is ``range(start, end)`` of span c; every crop is in exactly one of them, the lone-crop rule applies per clip and the outputs
        are scattered back to crop order.  ``after`` (``track_carry``): per clip the clip it continues (``plan_track_chains``), handed to
        the net where it can carry a state; the flat cut has none."""
        if members is None:
            members = [range(s, e) for s, e in split_clips(len(crops), max_clip_length)]
        run_u8 = getattr(self.keep_net, 'run_clips_u8', None)
        if run_u8 is None:
            x = crops_to_net_input(crops).unsqueeze(0).to(self.device)
            return [net_output_to_bgr_u8(f) for f in self._restore_clips(x, members)]
        crops = [np.asarray(c) for c in crops]
        kw = self._carry_kw(run_u8, after)
        # the reference net needs T>=2 (KP:173-178): a lone crop is duplicated and frame 0 kept.  The engine restores a lone frame as T=1
        # (same frame 0, half the work), and a net that takes ``after`` takes 1-frame clips as they are: it hands on the state after frame 0
        dup = 1 if (getattr(self.keep_net, 'supports_single_frame', False) or kw) else 2
        # (a clip = a list of crops: the engine copies them straight into its pinned upload buffer, no stacked intermediate)
        clips = [[crops[i] for i in m] * (dup if len(m) == 1 else 1) for m in members]
        outs = run_u8(clips, **kw)
        if outs is None:          # a non-root rank of a run sharded over several GPUs: rank 0 holds the frames and pastes
            return None
        faces = [None] * len(crops)
        for m, o in zip(members, outs):
            o = o.numpy()
            for k, i in enumerate(m):
                faces[i] = np.ascontiguousarray(o[k])
        return faces

    def _resizer(self, name):
        """The processor's resizer of class ``name`` (engine/resize.py: Lanczos4Resizer, AreaResizer, LinearResizer), built on first use."""
        rz = self._resizers.get(name)
        if rz is None:
            from ..engine import resize
            rz = self._resizers[name] = getattr(resize, name)(self.device)
        return rz

    def _gate(self, name):
        """Whether the HIP path ``name`` (a row of ``opencv_checks.GATES``, and the attribute of that name) stands in for cv2: forced by
        its environment variable or by whoever set the attribute, else decided once per processor -- by comparing the kernel with cv2
        itself where cv2 imports, and by the row's verdict without cv2."""
        if getattr(self, name) is None:
            check, without_cv2, no_cv2_text, failed_text = opencv_checks.GATES[name]
            try:
                _cv2()
            except ImportError:
                if no_cv2_text:
                    log.info(no_cv2_text)
                setattr(self, name, without_cv2)
                return without_cv2
            try:
                verdict = bool(getattr(opencv_checks, check)(self.device))
            except Exception as e:                      # no GPU / no library / any surprise: cv2 (the paste: the helper's own path)
                if failed_text:
                    log.info(failed_text, e)
                verdict = False
            setattr(self, name, verdict)
        return getattr(self, name)

    def _run_upscaler(self, model, cv2_image):
        if model is None:
            return cv2_image
        t = cv2_to_comfy_image(cv2_image).to(self.device).movedim(-1, -3)
        s = tiled_scale(t, lambda a: model.model(a), tile_x=512, tile_y=512, overlap=64,
                        upscale_amount=model.scale)
        return comfy_image_to_cv2(torch.clamp(s.movedim(-3, -1), min=0, max=1.0))

    def _final_background(self, frame_bgr, factor, on_device=False):
        """The background at the output size (face_restoration_helper.py:354-356).  ``on_device``: the consumer is the HIP paste, so
        a background the device resized stays there (a tensor); otherwise it is a host array."""
        up = self._run_upscaler(self.bg_upscale_model, frame_bgr)
        h, w, _ = frame_bgr.shape
        return self._lanczos(up, int(w * factor), int(h * factor), on_device)

    def _lanczos(self, img, w, h, on_device=False):
        """``_resize(img, w, h, 'INTER_LANCZOS4')``: identity returns ``img``; uint8 3-channel images go to the device kernel when
        ``_gate('gpu_resize')`` allows it, everything else (grey / 4-channel / other dtypes, an empty target) to cv2."""
        if img.shape[0] == h and img.shape[1] == w:
            return img
        if (w > 0 and h > 0 and len(img.shape) == 3 and img.shape[2] == 3 and img.dtype in (np.uint8, torch.uint8)
                and self._gate('gpu_resize')):
            out = self._resizer('Lanczos4Resizer').resize_u8(img, w, h)
            return out if on_device else out.cpu().numpy()
        return _resize(_host(img), w, h, 'INTER_LANCZOS4')

    def _lanczos_batch(self, frames, w, h):
        """``_lanczos`` over a uint8 [m,H,W,3] device batch that stays on the device: one launch on the current stream, identity returns
        ``frames``.  For callers that have settled ``_gate('gpu_resize')`` already (``_aligned_stream_applies``)."""
        if frames.shape[1] == h and frames.shape[2] == w:
            return frames
        return self._resizer('Lanczos4Resizer').resize_u8(frames, w, h)

    def _detect_resize_device(self, imgs, w2, h2):
        """uint8 [H,W,3] frames of one size -> the uint8 [n,h2,w2,3] detector batch on the device: every frame is copied straight into one
        [n,H,W,3] device tensor (no host stack; frames of the pinned conversion buffer copy asynchronously) and all of them are resized
        by one ``keep_resize_area_u8`` launch on the device's current stream.  The resized frames never exist on the host."""
        rz = self._resizer('AreaResizer')
        dev = rz.device
        h, w = imgs[0].shape[:2]
        with torch.cuda.device(dev):
            buf = torch.empty((len(imgs), h, w, 3), dtype=torch.uint8, device=dev)
            for i, im in enumerate(imgs):
                buf[i].copy_(im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im)), non_blocking=True)
            return rz.resize_u8(buf, w2, h2)

    def _detect_resize_stored(self, buf, w2, h2):
        """``_detect_resize_device`` over a chunk that is on the device already (the frame store's tensor): the launch alone."""
        rz = self._resizer('AreaResizer')
        with torch.cuda.device(buf.device):
            return rz.resize_u8(buf, w2, h2)

    def _detect_resize_applies(self, imgs, resize):
        """(w2, h2) when the device resize takes this chunk's detector inputs -- every frame uint8 [H,W,3] of one size whose short side
        exceeds ``resize``, a geometry the kernel takes (a whole-number scale on both axes is OpenCV's integer path: cv2), the path
        enabled -- else None."""
        if resize is None or not imgs or self.gpu_detect_resize is False:
            return None
        first = tuple(imgs[0].shape)
        if len(first) != 3 or first[2] != 3 or min(first[:2]) <= resize:
            return None
        if any(tuple(im.shape) != first or im.dtype not in (np.uint8, torch.uint8) for im in imgs):
            return None
        from ..engine.resize import area_geometry_refused
        h, w = first[:2]
        scale = resize / min(h, w)
        w2, h2 = int(w * scale), int(h * scale)
        if area_geometry_refused(h, w, h2, w2) or not self._gate('gpu_detect_resize'):
            return None
        return w2, h2

    def _aligned_resize_device(self, frames, out=None):
        """uint8 [H,W,3] / [n,H,W,3] (host or device) -> the 512 x 512 crops on the device: one ``keep_resize_linear_u8`` launch on the
        current stream (into ``out`` where given)."""
        return self._resizer('LinearResizer').resize_u8(frames, 512, 512, out=out)

    def _aligned_face(self, img):
        """``_resize(img, 512, 512, 'INTER_LINEAR')`` of an aligned input: identity returns ``img``; a uint8 [H,W,3] image goes to the
        device kernel when ``_gate('gpu_aligned_resize')`` allows it and comes back as a host array; everything else (grey / 4-channel /
        other dtypes, an empty image, the path off) goes to cv2.  A device failure is logged and turns the path off."""
        if img.shape[0] == 512 and img.shape[1] == 512:
            return img
        if (len(img.shape) == 3 and img.shape[2] == 3 and img.dtype == np.uint8 and img.shape[0] > 0 and img.shape[1] > 0
                and self._gate('gpu_aligned_resize')):
            try:
                return self._aligned_resize_device(img).cpu().numpy()
            except Exception as e:
                log.warning("device resize of the aligned input failed (%s): cv2.resize", e)
                self.gpu_aligned_resize = False
        return _resize(img, 512, 512, 'INTER_LINEAR')

    def _enlarged_hw(self, h, w):
        """(H2, W2) ``read_image`` gives an [h,w] frame whose short side is below 512, else None."""
        f = small_frame_factor(h, w)
        if f is None:
            return None
        from ..engine.resize import LinearResizer
        w2, h2 = LinearResizer.enlarged_size(h, w, f, f)
        return h2, w2

    def _small_frames_probe(self, store, n_frames, frame, img):
        """The probe of a sequence, on its first frame: ``read_image`` turned ``frame`` (uint8 [h,w,3], short side below 512) into ``img``,
        uint8 [rint(h f), rint(w f), 3].  Then -- the knob allowing, the Lanczos resize of the backgrounds on the device, both copies of
        the sequence within the store's cap -- the store takes the small-frame form (``store.small``) and True comes back."""
        if self.gpu_small_frames is False or frame.ndim != 3:
            return False
        h, w = frame.shape[:2]
        hw2 = self._enlarged_hw(h, w)
        if hw2 is None or not isinstance(img, np.ndarray) or img.dtype != np.uint8 or tuple(img.shape) != hw2 + (3,):
            return False
        if store.cap_bytes is not None and n_frames * (h * w + hw2[0] * hw2[1]) * 3 > store.cap_bytes:
            return False
        if not self._gate('gpu_resize') or not self._gate('gpu_small_frames'):
            return False
        store.small = (small_frame_factor(h, w),) + hw2
        return True

    def _prep_small_chunk(self, store, k, frames_bgr):
        """``_prep_detect_chunk`` of the small-frame form: the chunk's original frames are uploaded, one launch enlarges them, and the
        enlarged chunk is the detector batch (short side 512: no detector resize).  ``read_image`` is not called: the state it would leave
        is the enlarged frame -- here its device view, of which ``_replay_chunk`` needs the shape -- and the grey flag of the frame as it
        came.  None after a failure (``_frame_store_failed``): the present handling takes this chunk and the rest."""
        try:
            rz = self._resizer('LinearResizer')
            store.fill(k, frames_bgr)
            ebuf = store.enlarge(k, rz)
        except Exception as e:
            self._frame_store_failed(store, e)
            return None
        return [(ebuf[j], _is_gray(fr, threshold=10)) for j, fr in enumerate(frames_bgr)], ebuf

    # ------------------------------------------------------------------ single image
    @torch.no_grad()
    def process_image(self, cv2_image_orig: np.ndarray, final_upscale_factor: float, has_aligned: bool,
                      only_center_face: bool, draw_box: bool):
        helper = self.face_helper
        helper.upscale_factor = final_upscale_factor
        self._aa_begin()
        bg_img_final = self._final_background(cv2_image_orig, final_upscale_factor, on_device=not has_aligned)

        if has_aligned:
            face = self._aligned_face(cv2_image_orig)
            helper.is_gray = _is_gray(face, threshold=10)
            helper.cropped_faces = [face]
            crops = [face]
        else:
            helper.clean_all()
            helper.read_image(cv2_image_orig)
            if helper.get_face_landmarks_5(only_center_face=only_center_face, resize=640,
                                           eye_dist_threshold=5) == 0:
                return _host(bg_img_final)
            self._align_warp(helper)
            crops = list(helper.cropped_faces)
            if not crops:
                return _host(bg_img_final)

        # one face -> T=2 duplicate, keep frame 0; several faces -> one "clip" of T=#faces (KP:173-178)
        # (track clips: the faces of one picture are no sequence -- each is a clip of its own, restored like a lone face)
        if self._per_track and len(crops) > 1:      # (a single image has nothing to carry)
            faces = self._restore_crops_u8(crops, max_clip_length=1, members=[[i] for i in range(len(crops))])
        else:
            faces = self._restore_crops_u8(crops, max_clip_length=max(len(crops), 1))
        if faces is None:
            return None
        self.last_restored_faces = faces
        helper.restored_faces = [f.astype('uint8') for f in faces]

        if not has_aligned:
            helper.get_inverse_affine(None)
            out = self._paste(helper, bg_img_final, draw_box, src_hw=tuple(cv2_image_orig.shape[:2]))
        else:
            out = helper.restored_faces[0]
            if self.face_upscale_model:
                out = self._run_upscaler(self.face_upscale_model, out)
            side = int(512 * final_upscale_factor)
            out = self._lanczos(out, side, side)
        return out if out is not None else _host(bg_img_final)

    # ------------------------------------------------------------------ paste-back
    def _paste(self, helper, bg, draw_box, src_hw=None, weights=None):
        """``helper.paste_faces_to_input_image(upsample_img=bg, draw_box=..., face_upsampler=...)`` behind one call
        (face_restoration_helper.py:346-475).  With ``gpu_paste`` and the configuration the loader builds (use_parse=True,
        colour frame already at the output size, no box, no face upsampler, every crop at the helper's face size) the
        per-face masks, warps and the blend run on the MI355X (engine/paste.py); every other configuration -- and every
        helper that is not the reference's -- goes to the helper's own method.

        ``src_hw``: the size of the frame the background was made from.  Where ``read_image`` enlarged that frame (short side below 512)
        the background fails the size test alone; with the device resizes on it is brought to the enlarged size times the factor here
        (:357-358) and the GPU paste keeps the frame.

        ``weights`` (track lifetimes with ``track_fade``): per face its weight in the composite, which only the GPU paste takes
        (``keep_paste_face_w``); where the helper's own paste takes the frame a fade is ignored, with one logged warning."""
        wkw = {} if weights is None else {'weights': weights}        # (without a fade: today's calls, argument for argument)
        if self._gate('gpu_paste'):
            if self._gpu_paste_applies(helper, bg, draw_box):
                return self._paste_gpu(helper, bg, draw_box, **wkw)
            hw2 = self._enlarged_hw(*src_hw) if src_hw is not None and self.gpu_small_frames is not False else None
            if (hw2 is not None and tuple(getattr(getattr(helper, 'input_img', None), 'shape', ())[:2]) == hw2
                    and self._gpu_paste_applies(helper, bg, draw_box, size_test=False) and self._gate('gpu_resize')):
                up = getattr(helper, 'upscale_factor', 1)
                return self._paste_gpu(helper, self._lanczos(bg, int(hw2[1] * up), int(hw2[0] * up), on_device=True), draw_box, **wkw)
        self._fade_ignored(weights)
        self._aa_ignored()
        return helper.paste_faces_to_input_image(upsample_img=_host(bg), draw_box=draw_box, face_upsampler=self.face_upscale_model)

    def _aa_kw(self):
        """The keyword that turns the alias-free paste on in ``GpuPaster.paste`` -- nothing with the knob off: today's calls, argument for
        argument."""
        return {'aa': True} if getattr(self, 'paste_aa', False) else {}

    def _aa_begin(self):
        """A public call starts: ``last_paste_aa`` counts from nothing (with the knob off nothing is written)."""
        if getattr(self, 'paste_aa', False):
            self.last_paste_aa = {}

    def _aa_count(self, paster):
        """After ``paster.paste(**self._aa_kw())``: its faces into ``last_paste_aa``, {sub-samples per axis: faces}."""
        if getattr(self, 'paste_aa', False):
            seen = getattr(self, 'last_paste_aa', None)
            if seen is None:
                seen = self.last_paste_aa = {}
            for n in paster.last_aa or ():
                if n is not None:
                    seen[n] = seen.get(n, 0) + 1

    def _aa_ignored(self):
        """The helper's own paste takes one tap per pixel: the knob is dropped there, with one logged warning per processor."""
        if getattr(self, 'paste_aa', False) and not getattr(self, '_aa_warned', False):
            self._aa_warned = True
            log.warning("KEEP_AMD_PASTE_AA: the helper's own paste takes this frame; faces are pasted with the reference's single tap")

    def _fade_ignored(self, weights):
        """The helper's own paste has no per-face weight: a fade is dropped there, with one logged warning per processor."""
        if weights is not None and any(w != 1.0 for w in weights) and not getattr(self, '_fade_warned', False):
            self._fade_warned = True
            log.warning("KEEP_AMD_TRACK_FADE: the helper's own paste takes this frame; faces are pasted without a fade")

    def _align_warp(self, helper, keep_on_device=False):
        """``helper.align_warp_face()`` (face_restoration_helper.py:256-320).  With the GPU cv path and the default configuration
        (no pad_blur, constant border) only the similarity fit stays on the host (``cv2.estimateAffinePartial2D``, :305); the
        ``cv2.warpAffine`` that produces the 512 x 512 crops (:316-318) runs on the device (``keep_warp_affine_u8``)."""
        if (not self._gate('gpu_paste') or getattr(helper, 'pad_blur', False) or not hasattr(helper, 'face_template')
                or getattr(helper.input_img, 'dtype', None) != np.uint8):       # (16-bit sources are float64 after read_image)
            return helper.align_warp_face()
        from ..engine.paste import crop_faces
        fit = getattr(helper, 'estimate_similarity', None)          # (a helper may bring its own fit: bench.py's cv2-free stand-in)
        cv2 = _cv2() if fit is None else None
        mats = [fit(lm) if fit is not None else cv2.estimateAffinePartial2D(lm, helper.face_template, method=cv2.LMEDS)[0]
                for lm in helper.all_landmarks_5]
        crops = crop_faces(helper.input_img, mats, tuple(helper.face_size), self.device)
        helper.affine_matrices.extend(mats)
        if keep_on_device:                                          # the streamed sequence path: no PCIe round trip of the crops
            helper.cropped_faces.extend(crops[i] for i in range(len(mats)))
        else:
            crops = crops.cpu().numpy()
            helper.cropped_faces.extend(crops[i] for i in range(len(mats)))

    def _gpu_paste_applies(self, helper, bg, draw_box, size_test=True):
        faces, mats = getattr(helper, 'restored_faces', None), getattr(helper, 'inverse_affine_matrices', None)
        if self.face_upscale_model is not None:            # (draw_box is on the device since round 4: keep_draw_box)
            return False
        use_parse = getattr(helper, 'use_parse', False)
        if not use_parse and not getattr(self, '_gpu_paste_forced', False):
            # face_restoration_helper.py:386-415 (erode + GaussianBlur(k, 0) at data-dependent sizes): bit-equal to
            # oracle/paste_oracle.py, but ``opencv_agrees_with_gpu_paste`` compares only the parse-mask composite and the crop warp
            # with cv2 itself -- this branch stays opt-in (KEEP_AMD_GPU_PASTE=1) until it has been compared on an installation
            return False
        if (use_parse and getattr(helper, 'face_parse', None) is None) or not faces or mats is None:
            return False
        if len(faces) != len(mats):
            return False
        if isinstance(bg, torch.Tensor):                   # the background resized on the device (final_upscale_factor != 1)
            if bg.dtype != torch.uint8 or bg.dim() != 3 or bg.shape[2] != 3 or not bg.is_cuda:
                return False
        elif not isinstance(bg, np.ndarray) or bg.dtype != np.uint8 or bg.ndim != 3 or bg.shape[2] != 3:
            return False
        h, w = getattr(helper, 'input_img', bg).shape[:2]
        up = getattr(helper, 'upscale_factor', 1)
        if size_test and (int(h * up), int(w * up)) != tuple(bg.shape[:2]):   # :355-356 would resize the background first
            return False
        fw, fh = getattr(helper, 'face_size', (512, 512))
        # grey sources (is_gray: add_restored_face stored bgr2gray + AdaIN faces, [512,512]): the reference replicates the channel
        # BEFORE the warp and the parse input (cv2.cvtColor GRAY2BGR, :377-378,418-419), and so does _paste_gpu
        return (fh, fw) == (512, 512) and all(np.asarray(f).shape in ((512, 512, 3), (512, 512)) and np.asarray(f).dtype == np.uint8
                                              for f in faces)

    @torch.no_grad()
    def _paste_gpu(self, helper, bg, draw_box=False, weights=None):
        from ..engine import hiplib as L
        from ..engine.paste import GpuPaster
        if self._paster is None:
            self._paster = GpuPaster(self.device)
        faces = torch.from_numpy(np.ascontiguousarray(np.stack(
            [np.asarray(f) if np.asarray(f).ndim == 3 else np.repeat(np.asarray(f)[:, :, None], 3, axis=2)      # GRAY2BGR
             for f in helper.restored_faces]))).to(self.device)
        wkw = {} if weights is None else {'weights': list(weights)}
        wkw.update(self._aa_kw())                         # (knob off: nothing is added)
        if not getattr(helper, 'use_parse', False):       # :386-415 erosion mask instead of the parse mask
            out = self._paster.paste(bg, faces, list(helper.inverse_affine_matrices), None, getattr(helper, 'upscale_factor', 1), draw_box, **wkw)
            if out is None:                                # a face larger than the blur kernel takes: the helper's own path
                self._fade_ignored(weights)
                self._aa_ignored()
                return helper.paste_faces_to_input_image(upsample_img=_host(bg), draw_box=draw_box, face_upsampler=None)
            self._aa_count(self._paster)
            return out.cpu().numpy()
        # :418-424  BGR uint8 -> RGB float (x/255 - 0.5)/0.5, one face per ParseNet call like the reference
        x = torch.empty(faces.shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.call('keep_img2tensor', faces, x, faces.numel() // 3)
        engine = getattr(helper.face_parse, 'engine', None)
        if engine is not None:            # ParseNet on the HIP engine (engine/parsenet.py): all faces of the frame in one batch
            classes = engine.classes(x)
        else:
            classes = []
            for i in range(faces.shape[0]):
                logits = helper.face_parse(x[i:i + 1].permute(0, 3, 1, 2).contiguous())[0]
                classes.append(logits.argmax(dim=1).squeeze(0).to(torch.uint8))
            classes = torch.stack(classes)
        out = self._paster.paste(bg, faces, list(helper.inverse_affine_matrices), classes, getattr(helper, 'upscale_factor', 1), draw_box, **wkw)
        self._aa_count(self._paster)
        return out.cpu().numpy()

    # ------------------------------------------------------------------ streamed restore + paste (round 5)
    def _stream_applies(self, helper, frames_bgr, crops, draw_box):
        """The streamed form of steps 3 + 4 needs: the engine's net (``run_clips_u8`` with ``sink``), not inside a torch.distributed
        job, the GPU cv path (``_gate('gpu_paste')``), the parse-mask composite with ParseNet on the engine, no face upsampler, uint8
        colour frames of one size and 512 x 512 crops -- i.e. the configuration ``_gpu_paste_applies`` admits frame by frame, decided
        once for the sequence.  ``KEEP_AMD_STREAM_PASTE=0`` keeps the per-frame path."""
        if not self._stream_config_applies(helper) or uniform_u8_frames(frames_bgr) is None:
            return False
        if tuple(getattr(helper, 'face_size', (512, 512))) != (512, 512):
            return False
        return crops is None or all(tuple(c.shape) == (512, 512, 3) for c in crops)

    def _stream_config_applies(self, helper):
        """What ``_stream_applies`` asks of the configuration (everything but the frames and the crops)."""
        if not _sink_streaming(self.keep_net):
            return False
        if self.face_upscale_model is not None or not getattr(helper, 'use_parse', False):
            return False
        if getattr(getattr(helper, 'face_parse', None), 'engine', None) is None or not self._gate('gpu_paste'):
            return False
        return tuple(getattr(helper, 'face_size', (512, 512))) == (512, 512)

    def _restore_and_paste_streamed(self, frames_bgr, crops, affines, faces_per_frame, max_clip_length, factor, draw_box, pbar,
                                    as_u8, store=None, input_hw=None, plan=None, weights=None):
        """Steps 3 and 4 of ``process_image_sequence`` (keep_processor.py:263-304) as ONE pipeline on the GPU.

        ``run_clips_u8(sink=...)`` restores the clips in batch groups and hands each finished, range-checked group over as device
        tensors (a pool worker's share arrives in host memory, with its ParseNet class maps).  Whenever the next frames in order
        have all their faces, they are processed on a second stream: ParseNet over up to 32 faces across frames, then per frame the
        reference's arithmetic in the reference's order -- inverse affine from the helper (``get_inverse_affine``), face after face
        blended into the background (engine/paste.py) -- and the download of the finished frame (converted to the ComfyUI float RGB
        layout on the device unless ``as_u8``).  The compute stream meanwhile runs the next group's forward.

        With ``store`` (``_stored_sequence``) ``crops`` is the [n_crops,512,512,3] device tensor the batched warp wrote and the clips are
        views of it; the background of frame t is the store's frame (resized on the paste stream at ``factor != 1``), also for frames
        without faces, and a chunk of the store is released once its last frame has been emitted.  A small-frame store
        (``store.small``) holds the original frames: the background is brought to the enlarged size times the factor behind that.

        ``input_hw`` (without a store): per frame with faces the size ``read_image`` gave it.  Where that is not the frame's own -- small
        frames, enlarged at :182-184 -- the inverse affines live in the enlarged frame, and the background is resized to that size times
        the factor before the composite, the helper's own :357-358.

        ``plan`` (track clips): ``plan_track_clips``' (clips, slot_of) instead of the cut of the flat list.  Crop numbering, ``first``,
        ``affines`` and the paste order stay; a clip's position k is crop ``clips[c][k]``.  With a store the crop tensor is laid out by
        slot (``_stored_sequence``), so the clips still are views of it.

        ``weights`` (track lifetimes with ``track_fade``): per crop, in the order of ``affines``, the weight of its face in the composite
        (``GpuPaster.paste(weights=...)``); None: every face at 1.0, today's calls."""
        from ..engine import hiplib as L
        from ..engine.paste import GpuPaster
        from .clip_plan import clip_slot_spans
        helper, net, dev = self.face_helper, self.keep_net, cuda_device(self.device)
        if self._paster is None:
            self._paster = GpuPaster(dev)
        paster, engine = self._paster, helper.face_parse.engine
        n_frames, n_crops = len(frames_bgr), len(crops)
        first = [0]
        for k in faces_per_frame:
            first.append(first[-1] + k)
        # the clips as crop indices: the plan's, or the cut of the flat list -- the plan whose slots are the crop numbers themselves
        members = plan[0] if plan is not None else [range(s, e) for s, e in split_clips(n_crops, max_clip_length)]
        clips = []
        for m, (s0, s1) in zip(members, clip_slot_spans(members)):
            if store is not None:
                clips.append(crops[s0:s1])                            # a view of the sequence's crop tensor, which is laid out by slot
            elif all(isinstance(crops[i], torch.Tensor) and crops[i].is_cuda for i in m):
                clips.append(torch.stack([crops[i] for i in m]))      # warped on this GPU: restored without leaving it
            else:
                clips.append([crops[i].cpu().numpy() if isinstance(crops[i], torch.Tensor) else np.asarray(crops[i]) for i in m])
        pool = getattr(net, 'pool', None)
        if pool is not None and hasattr(pool, 'set_parser'):          # the workers parse what they restore
            pool.set_parser(engine)
        ready, classes = [None] * n_crops, [None] * n_crops
        keep_restored = self.keep_restored_faces
        ps = getattr(self, '_paste_stream', None)
        if ps is None:
            ps = self._paste_stream = torch.cuda.Stream(device=dev)
        st, out = {'next': 0, 'aff': 0}, _HostOutput(n_frames, as_u8, dev)

        def on_dev(t):
            return t if (isinstance(t, torch.Tensor) and t.is_cuda) else torch.as_tensor(t).to(dev, non_blocking=True)

        def advance():
            f0 = f1 = st['next']
            while f1 < n_frames and all(ready[i] is not None for i in range(first[f1], first[f1 + 1])):
                f1 += 1
            if f1 == f0:
                return
            with torch.cuda.device(dev), torch.cuda.stream(ps):
                need = [i for i in range(first[f0], first[f1]) if classes[i] is None]
                for b0 in range(0, len(need), 32):                     # ParseNet across frames, <= 32 faces per call
                    idx = need[b0:b0 + 32]
                    fb = torch.stack([on_dev(ready[i]) for i in idx])
                    x = torch.empty(fb.shape, dtype=torch.float32, device=dev)
                    L.call('keep_img2tensor', fb, x, fb.numel() // 3)     # :418-422 BGR u8 -> RGB float (x / 255 - 0.5) / 0.5
                    cl = engine.classes(x)
                    for k, i in enumerate(idx):
                        classes[i] = cl[k]
                for t in range(f0, f1):
                    if store is not None:
                        bg = store.frame(t, ps)
                        bg = self._lanczos(bg, int(bg.shape[1] * factor), int(bg.shape[0] * factor), on_device=True)
                        if store.small is not None:
                            bg = self._lanczos(bg, int(store.small[2] * factor), int(store.small[1] * factor), on_device=True)
                    else:
                        bg = self._final_background(frames_bgr[t], factor, on_device=True)   # (factor != 1: resized on this stream)
                        hw = input_hw[t] if input_hw is not None else None
                        if hw is not None and tuple(hw) != tuple(frames_bgr[t].shape[:2]):
                            bg = self._lanczos(bg, int(hw[1] * factor), int(hw[0] * factor), on_device=True)
                    k = faces_per_frame[t]
                    if k == 0:
                        out.emit(t, (bg if isinstance(bg, torch.Tensor) else on_dev(np.ascontiguousarray(bg)))[None])
                        if store is not None and t + 1 == store.spans[t // store.chunk][1]:
                            store.release(t // store.chunk, ps)
                        continue
                    helper.affine_matrices = affines[st['aff']:st['aff'] + k]
                    helper.upscale_factor = factor
                    helper.get_inverse_affine(None)
                    wkw = {} if weights is None else {'weights': weights[st['aff']:st['aff'] + k]}
                    wkw.update(self._aa_kw())              # (knob off: nothing is added)
                    st['aff'] += k
                    ids = range(first[t], first[t + 1])
                    faces = torch.stack([on_dev(ready[i]) for i in ids])
                    cls = torch.stack([on_dev(classes[i]) for i in ids])
                    out.emit(t, paster.paste(bg, faces, list(helper.inverse_affine_matrices), cls, factor, draw_box, **wkw)[None])
                    self._aa_count(paster)
                    pbar.update(1)
                    if store is not None and t + 1 == store.spans[t // store.chunk][1]:
                        store.release(t // store.chunk, ps)             # (the allocator waits for this stream's reads)
                if not keep_restored:                                  # a long video must not hold every restored crop in HBM until the end
                    for i in range(first[f0], first[f1]):
                        ready[i], classes[i] = _EMITTED, None
            st['next'] = f1

        def sink(ids, crops_list, classes_list):
            for j, cid in enumerate(ids):
                for k, i in enumerate(members[cid]):
                    ready[i] = crops_list[j][k]
                    if classes_list is not None:
                        classes[i] = classes_list[j][k]
            advance()

        max_b = None
        groups = int(os.environ.get('KEEP_AMD_STREAM_GROUPS', '0') or 0)      # >= 2: at least that many batch groups (more overlap, smaller batches)
        if groups >= 2 and hasattr(net, 'clips_per_call'):
            cap = net.clips_per_call(max_clip_length, 512, 512)
            max_b = max(1, min(cap, -(-len(clips) // groups)))
        import inspect
        try:
            params = inspect.signature(net.run_clips_u8).parameters
        except (TypeError, ValueError):
            params = {}
        takes_all = any(p.kind == inspect.Parameter.VAR_KEYWORD for p in params.values())
        kw = {k: v for k, v in (('max_b', max_b), ('parse', True)) if takes_all or k in params}    # decided by capability, not by catching
        if plan is not None and len(plan) > 2:                         # track carry: per clip the clip it continues
            kw.update(self._carry_kw(net.run_clips_u8, plan[2]))
        net.run_clips_u8(clips, sink=sink, **kw)                                                     # a TypeError from inside the forward
        advance()                                                      # frames without faces behind the last restored one
        ps.synchronize()
        if st['next'] != n_frames:
            raise RuntimeError(f"streamed paste-back: {n_frames - st['next']} frame(s) never became ready")
        pbar.update(n_frames)
        # the restored crops stay on the GPU only on request (tests / tools: ``keep_restored_faces``, KEEP_AMD_KEEP_RESTORED=1); by default
        # each crop is released once its frame has been composited and nothing of the sequence outlives the call in HBM
        self.last_restored_faces = _DeviceFaces(ready) if keep_restored else []
        return out.out

    # ------------------------------------------------------------------ streamed aligned sequence
    def _aligned_stream_applies(self, frames_bgr, factor):
        """The device-resident form of an aligned sequence (``_aligned_streamed``) needs: the engine's net (``run_clips_u8`` with
        ``sink``) in one process without a worker pool (a pool worker's share arrives in host memory: the per-frame path keeps that
        case), not inside a torch.distributed job, no face / background upscale model, uint8 colour frames of one size, and the device
        path of every resize the call makes: ``_gate('gpu_resize')`` when the output size differs from its source's,
        ``_gate('gpu_aligned_resize')`` when the frames are not 512 x 512.  ``KEEP_AMD_STREAM_PASTE=0`` keeps the per-frame path."""
        net = self.keep_net
        if not _sink_streaming(net):
            return False
        if getattr(net, 'pool', None) is not None or self.face_upscale_model is not None or self.bg_upscale_model is not None:
            return False
        hw = uniform_u8_frames(frames_bgr)
        if hw is None or hw[0] <= 0 or hw[1] <= 0:
            return False
        h, w = hw
        src = (512, 512) if self.return_restored_aligned else (w, h)
        dst = (int(src[0] * factor), int(src[1] * factor))
        if dst[0] <= 0 or dst[1] <= 0 or (dst != src and not self._gate('gpu_resize')):
            return False
        return (h, w) == (512, 512) or bool(self._gate('gpu_aligned_resize'))

    def _aligned_streamed(self, frames_bgr, max_clip_length, factor, pbar, as_u8, scene=False):
        """Steps 2 - 4 of an aligned sequence (keep_processor.py:250-291 of the reference) with the frames resident on the GPU.

        The frames are uploaded in chunks of at most ``KEEP_AMD_DETECT_BATCH``, each frame copied straight into the chunk's [n,H,W,3]
        device tensor, and one ``keep_resize_linear_u8`` launch per chunk writes the chunk's 512 x 512 crops into the crop tensor of the
        sequence (frames that are 512 x 512 are copied into it and nothing is launched).  The clips are views of that tensor, so
        ``run_clips_u8(sink=...)`` neither stages nor uploads them.  The sink builds the output of every finished run of frames on the
        device: by default (reference quirk P2: the restored faces are not used) the input frames at the output size, one batched
        Lanczos launch per chunk; with ``return_restored_aligned`` the restored crops at ``int(512 * factor)``, one launch per run.
        All of it is queued on the stream the forward runs on -- the restored crops are consumed on their producing stream -- and
        only the finished output crosses PCIe (float RGB via ``keep_bgr_u8_to_comfy`` unless ``as_u8``).  Returns None, before anything
        was restored, when the device resize fails.

        ``scene`` (scene cuts): every uploaded chunk's signatures are taken on the device, from the frames as given, and the spans are
        cut per scene; nothing is carried across a cut."""
        from ..engine import hiplib as L
        net, dev = self.keep_net, cuda_device(self.device)
        n = len(frames_bgr)
        h, w = frames_bgr[0].shape[:2]
        restored_out = bool(self.return_restored_aligned)
        src_w, src_h = (512, 512) if restored_out else (w, h)
        out_w, out_h = int(src_w * factor), int(src_h * factor)
        chunk = max(1, int(os.environ.get('KEEP_AMD_DETECT_BATCH', '32') or 32))
        starts = list(range(0, n, chunk))
        keep_frames = not restored_out            # P2: the output is made of the input frames
        with torch.cuda.device(dev):
            crops = torch.empty((n, 512, 512, 3), dtype=torch.uint8, device=dev)
            sig_dev = torch.empty((n, 256), dtype=torch.int32, device=dev) if scene else None
            frames_dev = []                       # per chunk: its [m,H,W,3] input frames on the device (None once emitted / unused)
            for a in starts:
                part = frames_bgr[a:a + chunk]
                buf = crops[a:a + len(part)] if (h, w) == (512, 512) else torch.empty((len(part), h, w, 3), dtype=torch.uint8, device=dev)
                for i, fr in enumerate(part):
                    buf[i].copy_(torch.from_numpy(np.ascontiguousarray(fr)), non_blocking=True)
                if sig_dev is not None:
                    try:
                        L.call('keep_frame_signature_u8', buf, len(part), h, w, sig_dev[a:a + len(part)])
                    except Exception as e:              # logged, and the host function takes the signatures: the same integers
                        log.warning("frame signatures on the device failed (%s): the host function", e)
                        sig_dev = None
                if (h, w) != (512, 512):
                    try:
                        self._aligned_resize_device(buf, out=crops[a:a + len(part)])
                    except Exception as e:              # logged, and the per-frame path (cv2) takes the sequence and every later one
                        log.warning("device resize of the aligned frames failed (%s): cv2.resize", e)
                        self.gpu_aligned_resize = False
                        return None
                frames_dev.append(buf if keep_frames else None)
        spans = split_clips(n, max_clip_length)
        chain = [None] + list(range(len(spans) - 1))                                          # track carry: one track, its spans chained in order
        cuts = self._scene_cuts_of(frames_bgr, sig_dev) if scene else None
        if cuts:                                                                              # per scene: its own spans, its own chain
            from .scene_cuts import segments
            spans, chain = [], []
            for a, b in segments(n, cuts):
                for j, (s, e) in enumerate(split_clips(b - a, max_clip_length)):
                    chain.append(None if j == 0 else len(spans) - 1)
                    spans.append((a + s, a + e))
        t1_ok = getattr(net, 'supports_single_frame', False)
        carry_kw = self._carry_kw(net.run_clips_u8, chain)
        t1_ok = t1_ok or bool(carry_kw)
        clips = [crops[s:e] if (e - s > 1 or t1_ok) else torch.cat([crops[s:e], crops[s:e]]) for s, e in spans]   # (T >= 2: KP:173-178)
        restored = [None] * n
        keep_restored = self.keep_restored_faces
        st, out = {'next': 0}, _HostOutput(n, as_u8, dev)

        def advance():
            f0 = f1 = st['next']
            while f1 < n and restored[f1] is not None:
                f1 += 1
            if f1 == f0:
                return
            with torch.cuda.device(dev):           # (the current stream: the one the forward that produced the crops was queued on)
                if restored_out:
                    faces = torch.stack([restored[i] for i in range(f0, f1)])
                    out.emit(f0, self._lanczos_batch(faces, out_w, out_h))
                else:
                    for c in range(f0 // chunk, (f1 - 1) // chunk + 1):
                        a, b = max(f0, c * chunk), min(f1, (c + 1) * chunk)
                        out.emit(a, self._lanczos_batch(frames_dev[c][a - c * chunk:b - c * chunk], out_w, out_h))
                        if b == min(n, (c + 1) * chunk):
                            frames_dev[c] = None                       # the chunk's frames are released once all of them are out
            if not keep_restored:
                for i in range(f0, f1):
                    restored[i] = _EMITTED
            st['next'] = f1

        def sink(ids, crops_list, classes_list):
            for j, cid in enumerate(ids):
                s, e = spans[cid]
                for k in range(e - s):
                    restored[s + k] = crops_list[j][k]
            advance()

        net.run_clips_u8(clips, sink=sink, **carry_kw)
        torch.cuda.current_stream(dev).synchronize()
        if st['next'] != n:
            raise RuntimeError(f"streamed aligned sequence: {n - st['next']} frame(s) never became ready")
        pbar.update(n)
        self.last_restored_faces = _DeviceFaces(restored) if keep_restored else []
        return out.out

    # ------------------------------------------------------------------ sequence
    def _frame_store_begin(self, frames_bgr):
        """An empty ``_FrameStore`` for this sequence where the store applies, else None: where the streamed paste applies
        (``_stream_config_applies``) without a worker pool and without a background upscale model, with the device crop warp of
        ``_align_warp`` (no pad_blur, a face template), a detector that takes batches, uniform uint8 frames within the cap
        (``frame_store_plan``).  KEEP_AMD_FRAME_STORE=0 or an earlier failure of this processor: None."""
        if os.environ.get('KEEP_AMD_FRAME_STORE', '1') == '0' or not self.frame_store:
            return None
        helper, net = self.face_helper, self.keep_net
        use_batch, chunk = self._detect_batching(getattr(helper, 'face_detector', None), len(frames_bgr))
        if not use_batch or getattr(net, 'pool', None) is not None or self.bg_upscale_model is not None:
            return None
        if getattr(helper, 'pad_blur', False) or not hasattr(helper, 'face_template') or not self._stream_config_applies(helper):
            return None
        cap = int(_env_number('KEEP_AMD_FRAME_STORE_GB', FRAME_STORE_DEFAULT_GB, float) * 1e9)
        spans = frame_store_plan(frames_bgr, cap, chunk)
        if spans is None or torch.device(self.device).type != 'cuda':
            return None
        h, w = uniform_u8_frames(frames_bgr)            # (not None: the plan asked the same)
        return _FrameStore(spans, h, w, cuda_device(self.device), cap_bytes=cap)

    def _frame_store_failed(self, store, err):
        """A raised error while filling the store or in the batched warp (nothing has been restored yet): logged once, the store is off
        for this processor from here on, and the sequence takes the present path."""
        log.warning("keeping the frames on the device failed (%s): the per-frame upload path", err)
        self.frame_store = False
        store.dead = True
        store.drop()

    def _stored_sequence(self, store, frames_bgr, tracks, max_clip_length, factor, draw_box, pbar, as_u8, fade=None):
        """Steps 2 - 4 of a detected sequence over its frame store: the similarity matrices are fitted on the host as in ``_align_warp``
        (``read_image`` is not called again: the pre-pass showed that it leaves these frames as they are, or enlarges them the way the store
        did), ONE ``keep_warp_affine_batch_u8``
        call per chunk writes that chunk's crops straight into the sequence's [n_crops,512,512,3] crop tensor, and
        ``_restore_and_paste_streamed`` restores views of that tensor and pastes onto the stored frames.  None -- the present path takes
        the sequence -- when no frame has a face or when the warp fails (``_frame_store_failed``), and for small frames when ANY frame has
        no face: that frame's output has the original size, the others the enlarged one, which is the present path's to deal with."""
        helper = self.face_helper
        n_frames = len(frames_bgr)
        try:
            from ..engine.paste import crop_faces_batch
            fit = getattr(helper, 'estimate_similarity', None)      # (a helper may bring its own fit: bench.py's cv2-free stand-in)
            cv2 = _cv2() if fit is None else None
            per_frame = []
            for i in tqdm(range(n_frames), desc="Cropping and aligning faces"):
                active = [seq[i] for seq in tracks.values() if not np.isnan(seq[i]).any()]
                per_frame.append([fit(lm) if fit is not None else cv2.estimateAffinePartial2D(lm, helper.face_template, method=cv2.LMEDS)[0]
                                  for lm in active])
            faces_per_frame = [len(m) for m in per_frame]
            n_crops = sum(faces_per_frame)
            if n_crops == 0 or (store.small is not None and 0 in faces_per_frame):
                store.drop()
                return None
            plan = self._track_plan([[key for key, seq in tracks.items() if not np.isnan(seq[i]).any()] for i in range(n_frames)],
                                    max_clip_length) if self._per_track else None
            with torch.cuda.device(store.device):
                crops = torch.empty((n_crops, 512, 512, 3), dtype=torch.uint8, device=store.device)
                off = 0
                for k, (a, b) in enumerate(store.spans):
                    frame_of = [t - a for t in range(a, b) for _ in per_frame[t]]
                    mats = [M for t in range(a, b) for M in per_frame[t]]
                    if mats and plan is not None:        # track clips: the crop tensor is laid out by slot, crop i lives in slot_of[i]
                        crop_faces_batch(store.warp_source(k), frame_of, mats, crops, (512, 512), slot_of=plan[1][off:off + len(mats)])
                        off += len(mats)
                    elif mats:
                        crop_faces_batch(store.warp_source(k), frame_of, mats, crops[off:off + len(mats)], (512, 512))
                        off += len(mats)
                    store.ebufs[k] = None                # (an enlarged chunk has no reader behind its warp, which ran on its own stream)
        except Exception as e:
            self._frame_store_failed(store, e)
            return None
        affines = [M for ms in per_frame for M in ms]
        try:
            return self._restore_and_paste_streamed(frames_bgr, crops, affines, faces_per_frame, max_clip_length, factor, draw_box, pbar,
                                                    as_u8, store=store, plan=plan, weights=self._fade_of(tracks, fade, n_frames))
        finally:
            store.drop(getattr(self, '_paste_stream', None))        # (nothing is left after ``ps.synchronize()``; an error's way out: the paste stream may still read)

    @staticmethod
    def _fade_of(tracks, fade, n_frames):
        """``fade`` (``fade_weights``: per track key the weight of every frame) -> the paste weight of every crop, frame-major and in face
        order like ``affines``; None without a fade."""
        if fade is None:
            return None
        return [float(fade[key][i]) for i in range(n_frames) for key, seq in tracks.items() if not np.isnan(seq[i]).any()]

    def _track_plan(self, presence, max_clip_length):
        """``plan_track_clips`` for a sequence (``track_clips`` only): (clips as crop-index lists, slot of every crop); with
        ``track_carry`` ``plan_track_chains``: the same two and, per clip, the clip it continues."""
        from .clip_plan import plan_track_chains, plan_track_clips
        if self.track_carry:
            return plan_track_chains(presence, max_clip_length)
        return plan_track_clips(presence, max_clip_length)

    @property
    def _per_track(self):
        """Clips hold one track each: ``track_clips``, which ``track_carry``, ``scene_cuts`` and ``track_lifetimes`` imply (in the flat
        frame-major cut a clip spans the scene boundary, or the end of a lifetime, whatever the tracks do)."""
        return bool(self.track_clips or self.track_carry or getattr(self, 'scene_cuts', False) or getattr(self, 'track_lifetimes', False))

    # ------------------------------------------------------------------ scene cuts
    def _scene_cuts_apply(self, frames_bgr):
        """Whether this call looks for scene cuts: the knob, more than one frame, uniform uint8 [h,w,3] frames.  Anything else ignores the
        knob, with one logged warning."""
        if not getattr(self, 'scene_cuts', False):
            return False
        n = len(frames_bgr)
        if n < 2:
            self.last_scene_cuts, self.last_scene_distances = [], np.zeros((0,), np.float64)
            return False
        hw = uniform_u8_frames(frames_bgr)
        ok = hw is not None and hw[0] > 0 and hw[1] > 0
        if not ok:
            if not getattr(self, '_scene_warned', False):
                self._scene_warned = True
                log.warning("KEEP_AMD_SCENE_CUTS: the frames are not uint8 [h,w,3] of one size; no scene cuts")
            self.last_scene_cuts, self.last_scene_distances = [], np.zeros((0,), np.float64)
        return ok

    def _store_signatures(self, store, n_frames):
        """The device tensor the frame store's fills write their chunks' signatures into (``_FrameStore.fill``).  An allocation that
        fails leaves the store as it is: the host function takes the sequence."""
        try:
            with torch.cuda.device(store.device):
                store.sig = torch.empty((n_frames, 256), dtype=torch.int32, device=store.device)
        except Exception:
            store.sig = None

    def _scene_cuts_of(self, frames_bgr, sig_dev=None):
        """The cuts of this sequence -> sorted list of frames that open a scene; sets ``last_scene_cuts`` / ``last_scene_distances``.
        ``sig_dev``: the signatures where the kernel wrote them (ONE download), else ``frame_signature_host`` frame by frame: the same
        integers either way."""
        from .scene_cuts import find_cuts, frame_signature_host, signature_distances
        sigs = None
        if sig_dev is not None:
            try:
                sigs = sig_dev.cpu().numpy()
            except Exception as e:
                log.warning("reading the frame signatures back failed (%s): the host function", e)
        if sigs is None:
            sigs = np.stack([frame_signature_host(frames_bgr[i]) for i in range(len(frames_bgr))])
        h, w = frames_bgr[0].shape[:2]
        self.last_scene_distances = signature_distances(sigs, h * w)
        self.last_scene_cuts = find_cuts(sigs, h * w, self.scene_cut_threshold)
        return self.last_scene_cuts

    def _carry_kw(self, run, after):
        """{'after': after} where ``track_carry`` is on, some clip has a predecessor and ``run`` (the net's ``run_clips_u8``) takes the
        argument -- decided by capability; a net that cannot carry restores every clip from nothing, with one logged warning.  A net
        that takes ``after`` MUST take T = 1 clips, carried or not, whatever its ``supports_single_frame`` says: it is handed 1-frame
        clips as they are, never the host-side T = 2 duplicate: the duplicate rule is the net's
        then (``KeepNet``: carried 1-frame clips run as their duplicate inside the call), so the state handed on is the one after frame 0."""
        if not self.track_carry or after is None or all(p is None for p in after):
            return {}
        import inspect
        try:
            params = inspect.signature(run).parameters
        except (TypeError, ValueError):
            params = {}
        if 'after' in params or any(p.kind == inspect.Parameter.VAR_KEYWORD for p in params.values()):
            return {'after': list(after)}
        if not getattr(self, '_carry_warned', False):
            self._carry_warned = True
            log.warning("KEEP_AMD_TRACK_CARRY: this net cannot start a clip from a state; clips start from nothing")
        return {}

    def _detect_batching(self, det, n):
        """(whether the pre-pass runs the detector over batches, frames per chunk)"""
        helper = self.face_helper
        use_batch = hasattr(det, 'detect_batch') and getattr(helper, 'det_model', 'retinaface') != 'dlib' and n > 0
        return use_batch, (max(1, int(getattr(getattr(det, 'engine', None), 'max_frames', 32))) if use_batch else 1)

    def _detect_all(self, frames_bgr, only_center_face, store=None):
        """Landmarks of every frame (keep_processor.py:207-213: one ``get_face_landmarks_5`` call -- one detector forward and
        one host round trip -- per frame).  With the engine's detector (engine/retinaface.py, ``detect_batch``) the network
        runs over the video in chunks of the detector's batch axis (``KEEP_AMD_DETECT_BATCH`` frames: the host never holds more
        than two chunks of detector inputs, the one in the detector and the one being prepared -- a 3000-frame 1080p video would
        otherwise stack ~13 GB of resized frames; with a worker pool the chunks go out in windows of ``world`` chunks,
        ``_detect_all_pooled``, and the bound is two windows = 2 x world chunks); the
        helper's own per-frame host logic (resize rule, eye-distance filter, centre-face selection:
        face_restoration_helper.py:206-252) then runs unchanged on the stored detections of the chunk, on the SAME
        ``read_image`` result the detector input was built from, so the landmarks are what the per-frame loop produces."""
        raw = []
        helper = self.face_helper
        det = getattr(helper, 'face_detector', None)
        use_batch, chunk = self._detect_batching(det, len(frames_bgr))
        bar = tqdm(total=len(frames_bgr), desc="Detecting face landmarks")
        starts = list(range(0, len(frames_bgr), chunk))
        gpus = self._detection_pool(det, len(starts)) if use_batch else None
        if gpus is not None:
            self._detect_all_pooled(gpus, det, frames_bgr, only_center_face, chunk, starts, raw, bar)
            bar.close()
            return raw
        # Round 6: the detector's forward of chunk k (GPU, one worker thread: the launches and the D2H waits release the GIL) runs under the
        # HOST preparation of chunk k + 1 (read_image + the INTER_AREA resize of every frame: a third of the pre-pass) -- the same calls
        # on the same data in the same order per frame, only interleaved; KEEP_AMD_DETECT_OVERLAP=0: one after the other.  Where the device
        # resize applies (KEEP_AMD_GPU_DETECT_RESIZE, ``_prep_detect_chunk``) that host resize is gone: the chunk's frames are copied to the
        # device and resized there by one launch, stream-ordered behind the forward of chunk k
        pool = None
        if use_batch and len(starts) > 1 and os.environ.get('KEEP_AMD_DETECT_OVERLAP', '1') != '0':
            from concurrent.futures import ThreadPoolExecutor
            pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='keep-detect')
        try:
            # with a frame store (``_frame_store_begin``: same chunks) every chunk's frames stay on the device behind its detector input
            skw = (lambda k: {}) if store is None else (lambda k: dict(store=store, k=k))
            prepared = self._prep_detect_chunk(frames_bgr[starts[0]:starts[0] + chunk], self.detect_resize, **skw(0)) if use_batch else None
            for k, s in enumerate(starts):
                part = frames_bgr[s:s + chunk]
                states, batched = None, None
                if use_batch:
                    states, batch = prepared
                    fut = None
                    if batch is not None:
                        fut = pool.submit(det.detect_batch, batch, 0.97) if pool is not None else None
                        if fut is None:
                            batched = det.detect_batch(batch, 0.97)
                    if k + 1 < len(starts):                                # host work of the next chunk, under this chunk's forward
                        prepared = self._prep_detect_chunk(frames_bgr[starts[k + 1]:starts[k + 1] + chunk], self.detect_resize, **skw(k + 1))
                    if fut is not None:
                        batched = fut.result()
                self._replay_chunk(det, part, states, batched, only_center_face, raw, bar)
        finally:
            if pool is not None:
                pool.shutdown(wait=True)
        bar.close()
        return raw

    def _replay_chunk(self, det, part, states, batched, only_center_face, raw, bar):
        """The helper's per-frame host logic over one chunk of frames, in frame order: on the stored ``read_image`` state and the stored
        detections of the batched forward where there are any (``states`` / ``batched``), through the helper's own calls otherwise."""
        helper = self.face_helper
        for j, frame in enumerate(part):
            helper.clean_all()
            if states is not None:
                helper.input_img, helper.is_gray = states[j]       # what read_image(frame) left behind (:172-184)
            else:
                helper.read_image(frame)
            if batched is None:
                helper.get_face_landmarks_5(only_center_face=only_center_face, resize=self.detect_resize, eye_dist_threshold=5)
            else:
                helper.face_detector = _ReplayDetector(batched[j])
                try:
                    helper.get_face_landmarks_5(only_center_face=only_center_face, resize=self.detect_resize, eye_dist_threshold=5)
                finally:
                    helper.face_detector = det
            raw.append(list(helper.all_landmarks_5))
            bar.update(1)

    def _detection_pool(self, det, n_chunks):
        """The net's worker pool when the detection pre-pass can be spread over it: a live pool (``KEEP_AMD_GPUS``), a detector whose engine
        is of a kind the workers rebuild (``GpuPool.takes_detector``: RetinaFace; YOLOv5-face and dlib stay on the root) and more than one chunk.  KEEP_AMD_POOL_DETECT=0:
        never."""
        if n_chunks < 2 or os.environ.get('KEEP_AMD_POOL_DETECT', '1') == '0':
            return None
        gpus = getattr(self.keep_net, 'pool', None)
        if gpus is None or not hasattr(gpus, 'takes_detector') or getattr(gpus, 'closed', False):
            return None
        return gpus if gpus.takes_detector(getattr(det, 'engine', None)) else None

    def _detect_all_pooled(self, gpus, det, frames_bgr, only_center_face, chunk, starts, raw, bar):
        """``_detect_all`` over the worker pool (engine/pool.py:GpuPool.detect): the chunks are dispatched in windows of ``world`` chunks,
        chunk k of a window on rank k (the root's own on its GPU, under the workers' runs), and the host preparation of the next window
        runs under the current window's detection (KEEP_AMD_DETECT_OVERLAP=0: one after the other), so the root holds at most TWO windows
        of detector inputs.  A chunk without a batch (mixed sizes, non-uint8 frames) takes the per-frame path on the root.  The helper's
        per-frame host logic then replays on the root, in frame order, exactly as without a pool."""
        world = int(gpus.world)
        gpus.set_detector(det.engine)
        windows = [starts[i:i + world] for i in range(0, len(starts), world)]

        def prep(win):
            # (host batches: they cross to the workers through shared memory, so the device resize is not used here)
            return [self._prep_detect_chunk(frames_bgr[s:s + chunk], self.detect_resize, device_resize=False) for s in win]

        def forward(prepared):
            live = [batch for _, batch in prepared if batch is not None]
            flat = gpus.detect(live, 0.97) if live else []
            out, off = [], 0
            for _, batch in prepared:
                out.append(None if batch is None else flat[off:off + len(batch)])
                off += 0 if batch is None else len(batch)
            return out
        thread = None
        if len(windows) > 1 and os.environ.get('KEEP_AMD_DETECT_OVERLAP', '1') != '0':
            from concurrent.futures import ThreadPoolExecutor
            thread = ThreadPoolExecutor(max_workers=1, thread_name_prefix='keep-detect')
        try:
            prepared = prep(windows[0])
            for k, win in enumerate(windows):
                current = prepared
                fut = thread.submit(forward, current) if thread is not None else None
                batched = forward(current) if fut is None else None
                if k + 1 < len(windows):                                   # host work of the next window, under this window's detection
                    prepared = prep(windows[k + 1])
                if fut is not None:
                    batched = fut.result()
                for s, (states, _), res in zip(win, current, batched):
                    self._replay_chunk(det, frames_bgr[s:s + chunk], states, res, only_center_face, raw, bar)
                del current, batched
        finally:
            if thread is not None:
                thread.shutdown(wait=True)

    def _prep_detect_chunk(self, frames_bgr, resize, device_resize=True, store=None, k=None):
        """One chunk of frames: the helper state ``read_image`` leaves behind per frame (input image, grey flag) and the detector inputs
        ``get_face_landmarks_5`` would build from it (face_restoration_helper.py:206-216: frames whose short side exceeds ``resize`` are
        scaled down with INTER_AREA), stacked -> (states, batch).  ``batch`` is None when the frames differ in size or are not uint8
        (16-bit sources become float64 in ``read_image``: the per-frame path converts them the way the reference does).  Who resizes: a
        helper's own ``resize_for_detector`` first; else, with ``device_resize``, the HIP area resize over the whole chunk
        (``_detect_resize_applies``: the batch is then a device tensor); else ``_resize`` (cv2, on the host) frame by frame.

        ``store`` / ``k``: the sequence's frame store and this chunk's index in it.  Where ``read_image`` left every frame as it was, the
        frames are copied into the store's tensor of the chunk, which then is what the device resize reads, or -- frames that need no
        resize -- the detector batch itself.  A frame ``read_image`` changed ends the store quietly (the present path takes the
        sequence); a failing copy is logged and turns the store off for this processor.  The first frame of chunk 0 is the sequence's
        probe for small frames (``_small_frames_probe``): where ``read_image`` enlarged it the way :182-184 do, this chunk and every later
        one take ``_prep_small_chunk`` and ``read_image`` is not called again."""
        helper = self.face_helper
        own = getattr(helper, 'resize_for_detector', None)          # (a helper may bring its own resize: bench.py's cv2-free stand-in)
        if store is not None and not store.dead and store.small is not None:
            small = self._prep_small_chunk(store, k, frames_bgr)
            if small is not None:
                return small
        states = []
        for j, frame in enumerate(frames_bgr):
            helper.clean_all()
            helper.read_image(frame)
            states.append((helper.input_img, getattr(helper, 'is_gray', False)))
            if (j == 0 and k == 0 and store is not None and not store.dead and helper.input_img is not frame
                    and self._small_frames_probe(store, sum(b - a for a, b in store.spans), frame, helper.input_img)):
                small = self._prep_small_chunk(store, 0, frames_bgr)
                if small is not None:
                    return small
        imgs = [img for img, _ in states]
        buf = None
        if store is not None and not store.dead:
            if all(img is fr for img, fr in zip(imgs, frames_bgr)):
                try:
                    buf = store.fill(k, imgs)
                except Exception as e:
                    self._frame_store_failed(store, e)
            else:
                store.dead = True
        target = self._detect_resize_applies(imgs, resize) if own is None and device_resize else None
        if target is not None:
            try:
                return states, (self._detect_resize_device(imgs, *target) if buf is None else self._detect_resize_stored(buf, *target))
            except Exception as e:                      # logged, and the present path takes the chunk (and every later one)
                log.warning("device resize of the detector inputs failed (%s): cv2.resize", e)
                self.gpu_detect_resize = False
        if buf is not None and (resize is None or min(imgs[0].shape[:2]) <= resize):
            return states, buf                          # no detector resize: the stored chunk is the detector batch
        for i, img in enumerate(imgs):
            h, w = img.shape[:2]
            if resize is not None and min(h, w) > resize:
                scale = resize / min(h, w)
                img = (own(img, int(w * scale), int(h * scale)) if own is not None
                       else _resize(img, int(w * scale), int(h * scale), 'INTER_AREA' if scale < 1 else 'INTER_LINEAR'))
            imgs[i] = img if isinstance(img, torch.Tensor) else np.ascontiguousarray(img)
        if any(tuple(im.shape) != tuple(imgs[0].shape) or im.dtype not in (np.uint8, torch.uint8) for im in imgs):
            return states, None
        return states, (torch.stack(imgs) if isinstance(imgs[0], torch.Tensor) else np.stack(imgs))

    @torch.no_grad()
    def process_image_sequence(self, image_sequence_tensor: torch.Tensor, final_upscale_factor: float,
                               has_aligned_frames: bool, only_center_face: bool, draw_box: bool,
                               max_clip_length: int = 20):
        n_frames = image_sequence_tensor.shape[0]
        if n_frames == 0:
            return image_sequence_tensor
        # comfy_image_to_cv2 per frame (keep_processor.py:201,306 of the reference) -- on the device, chunked, under the detection pre-pass
        frames_bgr = frames_from_comfy(image_sequence_tensor, self.device)
        out = self._process_frames(frames_bgr, final_upscale_factor, has_aligned_frames, only_center_face, draw_box,
                                   max_clip_length, as_u8=False)
        if out is None:
            return None
        return out if isinstance(out, torch.Tensor) else (torch.cat([cv2_to_comfy_image(f) for f in out], dim=0) if out
                                                           else image_sequence_tensor)

    @torch.no_grad()
    def process_frames_u8(self, frames_bgr, final_upscale_factor: float = 1.0, has_aligned_frames: bool = False,
                          only_center_face: bool = True, draw_box: bool = False, max_clip_length: int = 20):
        """``process_image_sequence`` between its two ComfyUI converters: list of uint8 BGR frames -> uint8 BGR frames
        (a [N,H',W',3] tensor from the streamed paths -- ``_restore_and_paste_streamed``, ``_aligned_streamed`` --, a list of arrays
        otherwise).  What a video tool that already holds
        uint8 frames calls, and what bench.py times next to the float entry point."""
        return self._process_frames(list(frames_bgr), final_upscale_factor, has_aligned_frames, only_center_face, draw_box,
                                    max_clip_length, as_u8=True)

    def _process_frames(self, frames_bgr, final_upscale_factor, has_aligned_frames, only_center_face, draw_box,
                        max_clip_length, as_u8):
        n_frames = len(frames_bgr)
        pbar = ProgressBar(n_frames * 4)
        helper = self.face_helper
        self._aa_begin()

        # -- 1. landmarks per frame -> temporally smoothed tracks
        tracks, store, fade = {}, None, None             # fade (track lifetimes with ``track_fade``): per track key the paste weight of every frame
        scene = self._scene_cuts_apply(frames_bgr)      # (False with the knob off: nothing below computes, launches or writes anything new)
        cuts = None
        if not has_aligned_frames:
            store = self._frame_store_begin(frames_bgr)
            if scene and store is not None:
                self._store_signatures(store, n_frames)
            raw = self._detect_all(frames_bgr, only_center_face, store=store)
            if store is not None and (store.dead or not store.complete()):
                store.drop()
                store = None
            pbar.update(n_frames)
            if scene:
                cuts = self._scene_cuts_of(frames_bgr, store.sig if store is not None else None)
            smooth = smooth_center_face if only_center_face else smooth_tracked_faces
            life = {}
            if getattr(self, 'track_lifetimes', False):                     # (off: today's call, argument for argument)
                self.last_track_lifetimes = []
                life = {'lifetimes': max(0, int(self.track_max_gap)), 'report': self.last_track_lifetimes}
            tracks = smooth(raw, cuts, **life) if cuts else smooth(raw, **life)
            if life and int(getattr(self, 'track_fade', 0) or 0) > 0:
                fade = fade_weights(n_frames, self.last_track_lifetimes, int(self.track_fade), cuts)
            pbar.update(n_frames)
        else:
            pbar.update(n_frames * 2)

        # -- 2 - 4 of an aligned sequence with its frames resident on the device
        if has_aligned_frames and n_frames and self._aligned_stream_applies(frames_bgr, final_upscale_factor):
            out = self._aligned_streamed(frames_bgr, max_clip_length, final_upscale_factor, pbar, as_u8, scene=scene)
            if out is not None:                         # (None: the device resize failed and turned itself off)
                return out

        # -- 2 - 4 of a detected sequence whose frames the pre-pass left on the device
        if store is not None:
            out = self._stored_sequence(store, frames_bgr, tracks, max_clip_length, final_upscale_factor, draw_box, pbar, as_u8, fade=fade)
            if out is not None:                         # (None: no faces at all, or the batched warp failed and turned the store off)
                return out

        # -- 2. crops, flat and frame-major
        crops, affines, faces_per_frame, input_hw = [], [], [], [None] * n_frames
        stream_ok = (not has_aligned_frames) and self._stream_applies(helper, frames_bgr, None, draw_box)
        presence = [] if self._per_track else None      # track clips: the keys of the tracks behind every frame's crops, in face order
        weights = self._fade_of(tracks, fade, n_frames)     # None without a fade: per crop, in the order of ``affines``, its paste weight
        scene_of = None
        if scene and has_aligned_frames:                # an aligned sequence is one track per scene: its key is the scene's index
            from .scene_cuts import segments
            scene_of = [s for s, (a, b) in enumerate(segments(n_frames, self._scene_cuts_of(frames_bgr))) for _ in range(a, b)]
        for i in tqdm(range(n_frames), desc="Cropping and aligning faces"):
            if has_aligned_frames:
                frame_crops, frame_aff = [self._aligned_face(frames_bgr[i])], []
                if presence is not None:
                    presence.append([0 if scene_of is None else scene_of[i]])   # (one track on every frame: the plan is the cut of the flat list)
            else:
                frame_crops, frame_aff = [], []
                active = [seq[i] for seq in tracks.values() if not np.isnan(seq[i]).any()]
                if presence is not None:
                    presence.append([key for key, seq in tracks.items() if not np.isnan(seq[i]).any()])
                if active:
                    helper.clean_all()
                    helper.read_image(frames_bgr[i])
                    input_hw[i] = tuple(getattr(helper.input_img, 'shape', ())[:2]) or None
                    helper.all_landmarks_5 = active
                    self._align_warp(helper, keep_on_device=stream_ok)
                    frame_crops = list(helper.cropped_faces)
                    frame_aff = list(helper.affine_matrices)
            faces_per_frame.append(len(frame_crops))
            crops.extend(frame_crops)
            affines.extend(frame_aff)
            if presence is not None and len(presence[i]) != len(frame_crops):
                raise RuntimeError(f"track clips: frame {i} has {len(frame_crops)} crops for {len(presence[i])} tracks")
        plan = self._track_plan(presence, max_clip_length) if presence is not None else None

        # -- 3 + 4 streamed: restore group g+1 while group g is parsed, pasted and downloaded (round 5)
        # (small frames with a faceless frame: that frame keeps its size, the others are enlarged -- the streamed paste writes ONE output
        # tensor, so the per-frame path takes the sequence; with track lifetimes faceless frames are common)
        mixed = 0 in faces_per_frame and any(hw is not None and tuple(hw) != tuple(frames_bgr[i].shape[:2]) for i, hw in enumerate(input_hw))
        if crops and not has_aligned_frames and not mixed and self._stream_applies(helper, frames_bgr, crops, draw_box):
            return self._restore_and_paste_streamed(frames_bgr, crops, affines, faces_per_frame, max_clip_length,
                                                    final_upscale_factor, draw_box, pbar, as_u8, input_hw=input_hw, plan=plan, weights=weights)

        # -- 3. restore: the hot path
        crops = [c.cpu().numpy() if isinstance(c, torch.Tensor) else c for c in crops]
        restored_faces = []
        if crops:
            restored_faces = (self._restore_crops_u8(crops, max_clip_length) if plan is None
                              else self._restore_crops_u8(crops, max_clip_length, members=plan[0], after=plan[2] if len(plan) > 2 else None))
            if restored_faces is None:          # non-root rank of a sharded multi-GPU run (engine/dist.py): nothing to paste here
                return None
        self.last_restored_faces = restored_faces
        pbar.update(n_frames)

        # -- 4. paste back
        out_frames = []
        face_ptr = aff_ptr = 0
        for i in tqdm(range(n_frames), desc="Pasting faces and finalizing frames"):
            k = faces_per_frame[i]
            # (a background for the HIP paste may stay on the device; _paste downloads it if the helper's own paste takes the frame)
            bg = self._final_background(frames_bgr[i], final_upscale_factor,
                                        on_device=k > 0 and not has_aligned_frames and self.gpu_paste is not False)
            if has_aligned_frames and self.return_restored_aligned and k:
                # opt-in fix of reference quirk P2: an aligned sequence returns its restored faces, resized the way the
                # single-image node does (keep_processor.py:190-197), instead of the upscaled input
                face = restored_faces[face_ptr]
                face_ptr += k
                if self.face_upscale_model:
                    face = self._run_upscaler(self.face_upscale_model, face)
                side = int(512 * final_upscale_factor)
                out_frames.append(self._lanczos(face, side, side))
                continue
            if k == 0 or has_aligned_frames:            # aligned: restored faces unused (reference quirk P2)
                out_frames.append(bg)
                continue
            helper.restored_faces = [f.astype('uint8') for f in restored_faces[face_ptr:face_ptr + k]]
            helper.affine_matrices = affines[aff_ptr:aff_ptr + k]
            helper.upscale_factor = final_upscale_factor
            helper.get_inverse_affine(None)
            wkw = {} if weights is None else {'weights': weights[aff_ptr:aff_ptr + k]}      # (without a fade: today's call)
            out_frames.append(self._paste(helper, bg, draw_box, src_hw=tuple(frames_bgr[i].shape[:2]), **wkw))
            face_ptr += k
            aff_ptr += k
            pbar.update(1)

        return out_frames
