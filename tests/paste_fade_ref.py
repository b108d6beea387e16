"""The paste-back composite with a weight per face (keep_paste_face_w, GpuPaster.paste(weights=...)) restated in numpy, composed from
the exported parts of oracle/paste_oracle.py, which is imported unmodified: the restored face warped with ``warp_affine_u8``, the soft
mask from ``parse_soft_mask`` + ``warp_affine_f32`` (use_parse=True) or ``erosion_soft_mask`` (use_parse=False), and the blend of
``paste_faces`` (:463) with ONE float32 product added in front of it:

    soft = soft * weight
    frame = soft * face + (1 - soft) * frame

Every operation is a single, separately rounded float32 operation, as in the kernel, so the two agree bit for bit.  With every weight
1.0 the product is exact and this is ``paste_oracle.paste_faces`` (tests/test_track_lifetimes_host.py)."""
import numpy as np

import paste_oracle as P


def frame_soft_masks(upsample_img, restored_faces, inverse_affines, parse_classes=None, upscale_factor=1.0):
    """Per face the soft mask in frame space, float32 [H,W] (None for a skipped face): the weight-independent part, which the tests
    compute once and share."""
    h_up, w_up = upsample_img.shape[:2]
    out = []
    for idx, face in enumerate(restored_faces):
        M = inverse_affines[idx]
        if M is None:
            out.append(None)
        elif parse_classes is not None:
            out.append(P.warp_affine_f32(P.parse_soft_mask(parse_classes[idx]), M, w_up, h_up))
        else:
            out.append(P.erosion_soft_mask(M, w_up, h_up, upscale_factor, face.shape[:2])[0])
    return out


def composite_f32(upsample_img, restored_faces, inverse_affines, parse_classes=None, upscale_factor=1.0, weights=None, soft=None):
    """The float32 frame [H,W,3] behind the last face, before clip / round / uint8.  ``soft``: ``frame_soft_masks`` of the same
    arguments, where the caller already has them."""
    h_up, w_up = upsample_img.shape[:2]
    if soft is None:
        soft = frame_soft_masks(upsample_img, restored_faces, inverse_affines, parse_classes, upscale_factor)
    up = upsample_img.astype(np.float32)
    for idx, face in enumerate(restored_faces):
        M = inverse_affines[idx]
        if M is None:
            continue
        inv_restored = P.warp_affine_u8(face, M, w_up, h_up)
        w = np.float32(1.0 if weights is None else weights[idx])
        m = (soft[idx].astype(np.float32) * w)[:, :, None].astype(np.float32)
        up = m * inv_restored.astype(np.float32) + (np.float32(1) - m) * up
    return up


def paste_faces_weighted(upsample_img, restored_faces, inverse_affines, parse_classes=None, upscale_factor=1.0, weights=None, soft=None):
    """``paste_oracle.paste_faces`` (draw_box=False) with a weight per face -> uint8 [H,W,3]."""
    up = composite_f32(upsample_img, restored_faces, inverse_affines, parse_classes, upscale_factor, weights, soft)
    return np.round(np.clip(up, 0, 255)).astype(np.uint8)


def small_case(seed=3):
    """A 200 x 300 frame with two 512 x 512 faces mapped to boxes of about 90 px, the second cut by the frame's right and lower edge ->
    (frame uint8 [200,300,3], faces uint8 [2,512,512,3], crop -> frame matrices float64 [2,2,3], class maps uint8 [2,512,512])."""
    rng = np.random.default_rng(seed)
    frame = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)
    faces = rng.integers(0, 256, (2, 512, 512, 3), dtype=np.uint8)
    s = 90.0 / 512.0
    mats = np.array([[[s * np.cos(0.1), -s * np.sin(0.1), 40.3], [s * np.sin(0.1), s * np.cos(0.1), 50.7]],
                     [[s, 0.0, 251.6], [0.0, s, 139.2]]], np.float64)
    fy, fx = np.mgrid[0:512, 0:512].astype(np.float64)
    r = np.hypot((fx - 256) / 174.0, (fy - 266) / 215.0)
    cls = np.zeros((512, 512), np.uint8)
    cls[r < 1.15] = 17                                            # hair
    cls[r < 0.95] = 1                                             # skin
    cls[fy > 460] = 14                                            # neck
    return frame, faces, mats, np.stack([cls, cls[:, ::-1].copy()])
