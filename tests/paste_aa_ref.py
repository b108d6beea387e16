"""The alias-free paste-back composite (keep_paste_face_aa, GpuPaster.paste(aa=True)) restated in numpy, composed from the exported parts
of oracle/paste_oracle.py, which is imported unmodified.  Per face with N = ``aa_factor(M)`` sub-samples per axis:

    face sums   warp_affine_u8(face, ss_affine(M, N), N W, N H) -- the oracle's warp on the N-times finer frame grid -- reshaped to
                [H, N, W, N, 3] and summed as integers over the N x N cells
    mask sums   warp_affine_f32(parse_soft_mask(cls), ss_affine(M, N), N W, N H), every value quantised q = rint(s * 65536) (half to
                even, int32), summed likewise; use_parse=False: the frame-space ``erosion_soft_mask`` of M itself, as today
    blend       face = float32(S) * (1 / N^2), soft = float32(Q) * (1 / (65536 N^2)) -- exact: sums below 2^24, powers of two --, then
                tests/paste_fade_ref.py's  soft = soft * weight;  frame = soft * face + (1 - soft) * frame

Every sum is an integer sum and every float operation is one separately rounded float32 operation, as in the kernel, so the two agree bit
for bit.  With N = 1 everywhere this is ``paste_fade_ref.paste_faces_weighted`` (tests/test_paste_aa_host.py)."""
import numpy as np

import paste_oracle as P
from comfyui_keep_amd.engine.paste import aa_factor, ss_affine


def cell_sums(fine, N):
    """[N H, N W, ...] integers -> int32 [H, W, ...]: the sum over the N x N cell of every frame pixel."""
    H, W = fine.shape[0] // N, fine.shape[1] // N
    return fine.astype(np.int64).reshape((H, N, W, N) + fine.shape[2:]).sum(axis=(1, 3)).astype(np.int32)


def face_mean(face, M, N, W, H):
    """The area-sampled face in frame space, float32 [H,W,3]."""
    if N == 1:
        return P.warp_affine_u8(face, M, W, H).astype(np.float32)
    S = cell_sums(P.warp_affine_u8(face, ss_affine(M, N), N * W, N * H), N)
    return S.astype(np.float32) * np.float32(1.0 / (N * N))


def mask_mean(soft_face, M, N, W, H):
    """The area-sampled parse mask in frame space, float32 [H,W]; ``soft_face``: ``parse_soft_mask`` of the face's class map."""
    if N == 1:
        return P.warp_affine_f32(soft_face, M, W, H)
    s = P.warp_affine_f32(soft_face, ss_affine(M, N), N * W, N * H)
    q = np.rint(s.astype(np.float32) * np.float32(65536)).astype(np.int32)
    return cell_sums(q, N).astype(np.float32) * np.float32(1.0 / (65536 * N * N))


def frame_soft_masks(upsample_img, restored_faces, inverse_affines, parse_classes=None, upscale_factor=1.0, factors=None, parse_soft=None):
    """Per face the soft mask in frame space (None for a skipped face).  ``factors``: N per face (default: ``aa_factor`` of its matrix);
    ``parse_soft``: per face ``parse_soft_mask`` of its class map, where the caller already has it."""
    h_up, w_up = upsample_img.shape[:2]
    out = []
    for idx, face in enumerate(restored_faces):
        M = inverse_affines[idx]
        if M is None:
            out.append(None)
        elif parse_classes is not None:
            N = aa_factor(M) if factors is None else factors[idx]
            sf = P.parse_soft_mask(parse_classes[idx]) if parse_soft is None else parse_soft[idx]
            out.append(mask_mean(sf, M, N, w_up, h_up))
        else:
            out.append(P.erosion_soft_mask(M, w_up, h_up, upscale_factor, face.shape[:2])[0])
    return out


def composite_f32(upsample_img, restored_faces, inverse_affines, parse_classes=None, upscale_factor=1.0, weights=None, factors=None,
                  soft=None, means=None):
    """The float32 frame [H,W,3] behind the last face, before clip / round / uint8.  ``soft`` / ``means``: ``frame_soft_masks`` /
    per face ``face_mean`` of the same arguments, where the caller already has them."""
    h_up, w_up = upsample_img.shape[:2]
    if soft is None:
        soft = frame_soft_masks(upsample_img, restored_faces, inverse_affines, parse_classes, upscale_factor, factors)
    up = upsample_img.astype(np.float32)
    for idx, face in enumerate(restored_faces):
        M = inverse_affines[idx]
        if M is None:
            continue
        N = aa_factor(M) if factors is None else factors[idx]
        v = face_mean(face, M, N, w_up, h_up) if means is None else means[idx]
        w = np.float32(1.0 if weights is None else weights[idx])
        m = (soft[idx].astype(np.float32) * w)[:, :, None].astype(np.float32)
        up = m * v + (np.float32(1) - m) * up
    return up


def paste_faces_aa(upsample_img, restored_faces, inverse_affines, parse_classes=None, upscale_factor=1.0, weights=None, factors=None,
                   soft=None, means=None):
    """``GpuPaster.paste(aa=True)`` (draw_box=False) -> uint8 [H,W,3]."""
    up = composite_f32(upsample_img, restored_faces, inverse_affines, parse_classes, upscale_factor, weights, factors, soft, means)
    return np.round(np.clip(up, 0, 255)).astype(np.uint8)


def similarity(r, theta, tx, ty):
    """The crop -> frame matrix of scale r, rotation theta (rad) and translation (tx, ty), float64 [2,3]."""
    c, s = r * np.cos(theta), r * np.sin(theta)
    return np.array([[c, -s, tx], [s, c, ty]], np.float64)


def checkerboard_case(r, theta):
    """The case of the issue: a one-pixel checkerboard face (0 / 255) pasted at scale r, rotated by theta, onto a flat frame of value 40
    with an all-skin class map -> (frame uint8 [160,200,3], face uint8 [512,512,3], M, class map uint8 [512,512]).  The matrix is the
    scale and the rotation alone, no translation: the crop's corner sits on the frame's, and what the rotation or the scale pushes past
    the frame's edges is cut."""
    yy, xx = np.mgrid[0:512, 0:512]
    face = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    frame = np.full((160, 200, 3), 40, np.uint8)
    return frame, face, similarity(r, theta, 0.0, 0.0), np.ones((512, 512), np.uint8)
