"""``cv2.resize(img, (W2, H2), interpolation=cv2.INTER_LANCZOS4)`` for uint8 BGR frames on the MI355X -- the background resize of
``final_upscale_factor`` (face_restoration_helper.py:354-356; reference keep_processor.py:139-142,283-286).

The per-axis tables (OpenCV 4.x ``interpolateLanczos4`` in double / float, int16 coefficients at scale 2048) come from the
library's host C (``keep_lanczos4_tables``), are uploaded once per geometry and cached; the separable 8-tap filter over every frame
of a call is one launch of ``keep_resize_lanczos4_u8`` (csrc/keep_resize.hip).  Whether this equals cv2 itself on an installation is
decided at run time by the processor (``opencv_agrees_with_gpu_resize``); tests/cv_lanczos_ref.py is the independent restatement the
kernel is checked against bit for bit.
"""
import ctypes as C

import numpy as np
import torch

from . import hiplib as L


def lanczos4_tables(S, D):
    """(ofs int32 [D], coef int16 [D, 8]) of one axis, S source -> D destination pixels (host memory; no device needed)."""
    lib = L.load(check_device=False)
    ofs = np.empty(D, np.int32)
    coef = np.empty((D, 8), np.int16)
    rc = lib.keep_lanczos4_tables(int(S), int(D), ofs.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise L.KeepHipError(f"keep_lanczos4_tables failed (code {rc}): {lib.keep_last_error().decode()}", code=rc)
    return ofs, coef


class Lanczos4Resizer:
    """Device tables cached per (H, W, H2, W2): a video has one geometry, so they are built once.  One instance per processor."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._tables = {}

    def _device_tables(self, H, W, H2, W2):
        key = (H, W, H2, W2)
        t = self._tables.get(key)
        if t is None:
            xo, xc = lanczos4_tables(W, W2)
            yo, yc = lanczos4_tables(H, H2)
            t = tuple(torch.from_numpy(a).to(self.device) for a in (xo, xc, yo, yc))
            torch.cuda.current_stream(self.device).synchronize()     # (read later from whichever stream resizes)
            self._tables[key] = t
        return t

    def resize_u8(self, frames, W2, H2):
        """uint8 BGR frames [H,W,3] or [N,H,W,3] (numpy or tensor) -> uint8 [H2,W2,3] / [N,H2,W2,3] on the device.  At identity the
        input comes back as it is and nothing is launched (cv2.resize copies; ``_resize`` in the processor returns its input)."""
        W2, H2 = int(W2), int(H2)
        shape = tuple(frames.shape)
        if len(shape) not in (3, 4) or shape[-1] != 3:
            raise ValueError(f"resize_u8: expected [H,W,3] or [N,H,W,3] uint8 BGR frames, got shape {shape}")
        H, W = shape[-3], shape[-2]
        if (H, W) == (H2, W2):
            return frames
        x = torch.as_tensor(frames)
        if x.dtype != torch.uint8:
            raise ValueError(f"resize_u8: expected uint8 frames, got {x.dtype}")
        x = x.to(self.device, non_blocking=True).contiguous()
        batched = x.dim() == 4
        if not batched:
            x = x[None]
        N = x.shape[0]
        out = torch.empty((N, H2, W2, 3), dtype=torch.uint8, device=self.device)
        if N == 0:
            return out if batched else out[0]
        xo, xc, yo, yc = self._device_tables(H, W, H2, W2)
        with torch.cuda.device(self.device):
            L.call('keep_resize_lanczos4_u8', x, out, N, H, W, H2, W2, xo, xc, yo, yc)
        return out if batched else out[0]
