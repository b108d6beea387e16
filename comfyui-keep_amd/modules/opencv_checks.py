"""Does a HIP kernel that restates an OpenCV function reproduce cv2 itself on THIS installation?  One self-check per device path of
``keep_processor.py`` -- each compares the kernel with cv2 bit for bit on a few fixed cases and raises ImportError without cv2 -- and the
table (``GATES``) by which the processor decides a path once (``KEEPFaceProcessor._gate``).  Nothing here refers to the processor.
"""
import numpy as np
import torch


def opencv_agrees_with_gpu_paste(device):
    """True iff the HIP paste-back (engine/paste.py) reproduces OpenCV bit for bit on this installation: the composite
    of engine/synth.py's 1080p / 3-face case computed with cv2 calls in the order of face_restoration_helper.py:382,426-468
    against ``GpuPaster.paste``, and the :316-318 crop warp against ``crop_faces``.  Raises ImportError without cv2."""
    import cv2
    from ..engine import paste as gp
    from ..engine import synth
    frame, faces, mats, classes = synth.synth_paste_case()
    H, W = frame.shape[:2]
    up = frame
    lut = np.asarray(gp.MASK_COLORMAP, np.float32)
    for face, M, cls in zip(faces, mats, classes):
        inv_restored = cv2.warpAffine(face, M, (W, H))
        m = lut[cls.astype(np.int64)]
        m = cv2.GaussianBlur(cv2.GaussianBlur(m, (101, 101), 11), (101, 101), 11)
        t = gp.PARSE_BORDER
        m[:t, :] = 0; m[-t:, :] = 0; m[:, :t] = 0; m[:, -t:] = 0
        soft = cv2.warpAffine(m / np.float32(255.0), M, (W, H))[:, :, None]
        up = soft * inv_restored + (1 - soft) * up
    ref = np.round(np.clip(up, 0, 255)).astype(np.uint8)
    got = gp.GpuPaster(device).paste(frame, faces, list(mats), torch.from_numpy(classes)).cpu().numpy()
    if not np.array_equal(got, ref):
        return False
    fwd = cv2.invertAffineTransform(mats[2])
    crop = cv2.warpAffine(frame, fwd, (512, 512), borderMode=cv2.BORDER_CONSTANT, borderValue=gp.ALIGN_BORDER_BGR)
    return bool(np.array_equal(gp.crop_faces(frame, [fwd], device=device)[0].cpu().numpy(), crop))


def opencv_agrees_with_gpu_resize(device):
    """True iff the HIP Lanczos resize (engine/resize.py) reproduces ``cv2.resize(..., INTER_LANCZOS4)`` bit for bit on this
    installation: up- and down-scales of random frames, odd sizes, a geometry whose source coordinates land on whole pixels (the
    1e30 branch of interpolateLanczos4) and a one-pixel-wide output.  Raises ImportError without cv2."""
    import cv2
    from ..engine.resize import Lanczos4Resizer
    rz = Lanczos4Resizer(device)
    rng = np.random.default_rng(0)
    for (h, w), (h2, w2) in (((90, 160), (180, 320)), ((37, 53), (48, 68)), ((120, 200), (84, 140)), ((300, 9), (100, 3)),
                             ((64, 64), (256, 256)), ((31, 17), (15, 1))):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = cv2.resize(img, (w2, h2), interpolation=cv2.INTER_LANCZOS4)
        if not np.array_equal(rz.resize_u8(img, w2, h2).cpu().numpy(), ref):
            return False
    return True


def opencv_agrees_with_gpu_detect_resize(device):
    """True iff the HIP area resize (engine/resize.py:AreaResizer) reproduces ``cv2.resize(..., INTER_AREA)`` bit for bit on this
    installation: the detector-input geometries of 1080p and 720p video (short side to 640) and small frames with 2-3 taps, a scale
    below 1.2 and a whole-number scale on one axis only.  Raises ImportError without cv2."""
    import cv2
    from ..engine.resize import AreaResizer
    rz = AreaResizer(device)
    rng = np.random.default_rng(0)
    for (h, w), (h2, w2) in (((1080, 1920), (640, 1137)), ((720, 1280), (640, 1137)), ((54, 96), (32, 56)), ((45, 80), (40, 71)),
                             ((48, 64), (16, 21)), ((270, 480), (160, 284))):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = cv2.resize(img, (w2, h2), interpolation=cv2.INTER_AREA)
        if not np.array_equal(rz.resize_u8(img, w2, h2).cpu().numpy(), ref):
            return False
    return True


def opencv_agrees_with_gpu_aligned_resize(device):
    """True iff the HIP bilinear resize (engine/resize.py:LinearResizer) reproduces ``cv2.resize(..., INTER_LINEAR)`` bit for bit on this
    installation, at the aligned-face target of 512 x 512: an enlargement, a fractional shrink, the exact 2x shrink (INTER_AREA's 2 x 2
    path inside cv2.resize), a non-square source and a one-pixel-wide source.  Raises ImportError without cv2."""
    import cv2
    from ..engine.resize import LinearResizer
    rz = LinearResizer(device)
    rng = np.random.default_rng(0)
    for h, w in ((256, 256), (720, 720), (1024, 1024), (300, 400), (64, 1)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = cv2.resize(img, (512, 512), interpolation=cv2.INTER_LINEAR)
        if not np.array_equal(rz.resize_u8(img, 512, 512).cpu().numpy(), ref):
            return False
    return True


def opencv_agrees_with_gpu_small_frame_resize(device):
    """True iff the HIP bilinear enlargement (engine/resize.py:LinearResizer.enlarge_u8) reproduces ``cv2.resize(img, (0, 0), fx=f, fy=f,
    interpolation=cv2.INTER_LINEAR)`` with ``f = 512.0 / min(h, w)`` bit for bit on this installation: landscape, portrait and a
    one-pixel-high source.  Raises ImportError without cv2."""
    import cv2
    from ..engine.resize import LinearResizer
    rz = LinearResizer(device)
    rng = np.random.default_rng(0)
    for h, w in ((360, 480), (480, 270), (240, 426), (1, 7)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        f = 512.0 / min(h, w)
        ref = cv2.resize(img, (0, 0), fx=f, fy=f, interpolation=cv2.INTER_LINEAR)
        if not np.array_equal(rz.enlarge_u8(img, f, f).cpu().numpy(), ref):
            return False
    return True


# One row per device path that stands in for a cv2 call, under the name of the processor's tri-state attribute (the environment variable
# is KEEP_AMD_ + that name in upper case): the self-check -- named, and looked up in this module when the gate is decided, so a test can
# substitute it --, the verdict without cv2 (a resize has no other path there; the paste has the helper's own), and what is logged (info)
# without cv2 and after a self-check that raised (no GPU / no library / any surprise: cv2).  None: nothing is logged.
GATES = {
    'gpu_paste': ('opencv_agrees_with_gpu_paste', False, None, None),
    'gpu_resize': ('opencv_agrees_with_gpu_resize', True,
                   "cv2 is not installed: final_upscale_factor resizes run on the device (KEEP_AMD_GPU_RESIZE)",
                   "device Lanczos resize self-check failed (%s): cv2.resize"),
    'gpu_detect_resize': ('opencv_agrees_with_gpu_detect_resize', True,
                          "cv2 is not installed: detector inputs are resized on the device (KEEP_AMD_GPU_DETECT_RESIZE)",
                          "device area resize self-check failed (%s): cv2.resize"),
    'gpu_aligned_resize': ('opencv_agrees_with_gpu_aligned_resize', True,
                           "cv2 is not installed: aligned inputs are resized on the device (KEEP_AMD_GPU_ALIGNED_RESIZE)",
                           "device bilinear resize self-check failed (%s): cv2.resize"),
    'gpu_small_frames': ('opencv_agrees_with_gpu_small_frame_resize', True,
                         "cv2 is not installed: small frames are enlarged on the device (KEEP_AMD_GPU_SMALL_FRAMES)",
                         "device enlargement self-check failed (%s): cv2.resize"),
}
