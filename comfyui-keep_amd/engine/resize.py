"""``cv2.resize(img, (W2, H2), interpolation=cv2.INTER_LANCZOS4)`` for uint8 BGR frames on the MI355X -- the background resize of
``final_upscale_factor`` (face_restoration_helper.py:354-356; reference keep_processor.py:139-142,283-286).

The per-axis tables (OpenCV 4.x ``interpolateLanczos4`` in double / float, int16 coefficients at scale 2048) come from the
library's host C (``keep_lanczos4_tables``), are uploaded once per geometry and cached; the separable 8-tap filter over every frame
of a call is one launch of ``keep_resize_lanczos4_u8`` (csrc/keep_resize.hip).  Whether this equals cv2 itself on an installation is
decided at run time by the processor (``opencv_agrees_with_gpu_resize``); tests/cv_lanczos_ref.py is the independent restatement the
kernel is checked against bit for bit.

``cv2.resize(img, (W2, H2), interpolation=cv2.INTER_AREA)`` for frames that shrink on both axes -- the detector input of
face_restoration_helper.py:206-216 -- is the second resize here: ``area_tables`` (``keep_area_tables``, host C: OpenCV 4.x
``computeResizeAreaTab`` in CSR form) and ``AreaResizer`` (``keep_resize_area_u8``, csrc/keep_resize_area.hip, declared in the
extension header include/keep_cv_hip.h).  Its float32 sums are order-bound, so the kernel is built without FMA contraction;
tests/cv_area_ref.py is its restatement, and the processor's ``opencv_agrees_with_gpu_detect_resize`` decides on an installation.

``cv2.resize(img, (W2, H2), interpolation=cv2.INTER_LINEAR)`` -- the aligned-face input (keep_processor.py:158,250 of the reference) --
is the third: ``LinearResizer`` (``keep_resize_linear_u8``, csrc/keep_resize_linear.hip), any geometry, no tables: OpenCV's 11-bit fixed
point, and the 2 x 2 integer average cv2.resize substitutes at an exact 2x shrink.  tests/cv_linear_ref.py is its restatement, and
``opencv_agrees_with_gpu_aligned_resize`` decides on an installation.

``cv2.resize(img, (0, 0), fx=f, fy=f, interpolation=cv2.INTER_LINEAR)`` -- ``read_image``'s enlargement of a frame whose short side is
below 512 (face_restoration_helper.py:182-184) -- is the same kernel behind a second entry: ``LinearResizer.enlarge_u8``
(``keep_resize_linear_fxy_u8``).  The destination size is the rounded product, the coordinate scale is ``1 / f`` itself and there is no
2 x 2 substitution.  tests/cv_linear_fxy_ref.py is its restatement, and ``opencv_agrees_with_gpu_small_frame_resize`` decides on an
installation.
"""
import ctypes as C
import sys

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


def _frame_size(frames, who):
    """(H, W) of frames [H,W,3] or [N,H,W,3]; ``who`` (the method) opens the error text."""
    shape = tuple(frames.shape)
    if len(shape) not in (3, 4) or shape[-1] != 3:
        raise ValueError(f"{who}: expected [H,W,3] or [N,H,W,3] uint8 frames, got shape {shape}")
    return shape[-3], shape[-2]


class _Resizer:
    """What the three resizers share: the device, the conversion of a call's frames and output to what a launch takes, and device tables
    cached per (H, W, H2, W2) -- a video has one geometry, so they are built once."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._tables = {}

    def _device_tables(self, H, W, H2, W2):
        key = (H, W, H2, W2)
        t = self._tables.get(key)
        if t is None:
            t = tuple(torch.from_numpy(a).to(self.device) for a in self._axis_tables(W, W2) + self._axis_tables(H, H2))
            torch.cuda.current_stream(self.device).synchronize()     # (read later from whichever stream resizes)
            self._tables[key] = t
        return t

    def _input(self, frames, who):
        """(x, batched): frames of a checked shape as a contiguous uint8 [N,H,W,3] tensor on the device; ``batched``: they came with N."""
        x = torch.as_tensor(frames)
        if x.dtype != torch.uint8:
            raise ValueError(f"{who}: expected uint8 frames, got {x.dtype}")
        x = x.to(self.device, non_blocking=True).contiguous()
        batched = x.dim() == 4
        return (x if batched else x[None]), batched

    def _output(self, frames, H2, W2, out, who):
        """The [N,H2,W2,3] tensor a launch over ``frames`` (of a checked shape) writes: a new one, or ``out`` -- a contiguous uint8 tensor
        of the result's shape on this device -- seen with its N."""
        shape = tuple(frames.shape)
        N = shape[0] if len(shape) == 4 else 1
        if out is None:
            return torch.empty((N, H2, W2, 3), dtype=torch.uint8, device=self.device)
        want = shape[:-3] + (H2, W2, 3)
        if tuple(out.shape) != want or out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"{who}: out must be a contiguous uint8 {want} tensor on {self.device}")
        return out.view(N, H2, W2, 3)

    def _launch(self, entry, x, y, batched, *args):
        """One launch of ``entry`` over x [N,H,W,3] -> y [N,H2,W2,3] (none for N = 0); the result as the frames came, with or without N."""
        (N, H, W, _), (H2, W2) = x.shape, y.shape[1:3]
        if N > 0:
            with torch.cuda.device(self.device):
                L.call(entry, x, y, N, H, W, H2, W2, *args)
        return y if batched else y[0]


class Lanczos4Resizer(_Resizer):
    """``cv2.resize(..., INTER_LANCZOS4)`` for uint8 3-channel frames.  One instance per processor."""
    _axis_tables = staticmethod(lanczos4_tables)

    def resize_u8(self, frames, W2, H2):
        """uint8 BGR frames [H,W,3] or [N,H,W,3] (numpy or tensor) -> uint8 [H2,W2,3] / [N,H2,W2,3] on the device.  At identity the
        input comes back as it is and nothing is launched (cv2.resize copies; ``_resize`` in the processor returns its input)."""
        W2, H2 = int(W2), int(H2)
        H, W = _frame_size(frames, 'resize_u8')
        if (H, W) == (H2, W2):
            return frames
        x, batched = self._input(frames, 'resize_u8')
        y = self._output(x, H2, W2, None, 'resize_u8')
        tables = self._device_tables(H, W, H2, W2) if len(x) else ()      # (an empty batch builds none)
        return self._launch('keep_resize_lanczos4_u8', x, y, batched, *tables)


def area_tables(S, D):
    """(start int32 [D + 1], si int32 [n], alpha float32 [n]) of one axis of INTER_AREA, S source -> D < S destination pixels: the entries
    of destination d are ``start[d] .. start[d + 1]`` (host memory; no device needed)."""
    lib = L.load(check_device=False)
    S, D = int(S), int(D)
    cap = max(1, S + 2 * max(D, 0))                      # a head and a tail per destination, every source pixel once
    start = np.empty(max(D, 0) + 1, np.int32)
    si = np.empty(cap, np.int32)
    alpha = np.empty(cap, np.float32)
    rc = lib.keep_area_tables(S, D, cap, start.ctypes.data_as(C.c_void_p), si.ctypes.data_as(C.c_void_p), alpha.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise L.KeepHipError(f"keep_area_tables failed (code {rc}): {lib.keep_last_error().decode()}", code=rc)
    n = int(start[D])
    return start, si[:n].copy(), alpha[:n].copy()


def _whole_scale(S, D):
    scale = 1.0 / (float(D) / float(S))
    return abs(scale - int(scale)) < sys.float_info.epsilon


def area_geometry_refused(H, W, H2, W2):
    """Whether ``keep_resize_area_u8`` refuses [H,W] -> [H2,W2]: not a shrink on both axes, or a whole-number scale on both (OpenCV's
    integer INTER_AREA path, which the library does not restate)."""
    if H2 <= 0 or W2 <= 0 or H2 >= H or W2 >= W:
        return True
    return _whole_scale(H, H2) and _whole_scale(W, W2)


class AreaResizer(_Resizer):
    """``cv2.resize(..., INTER_AREA)`` for uint8 3-channel frames that shrink on both axes.  One instance per processor."""
    _axis_tables = staticmethod(area_tables)

    def resize_u8(self, frames, W2, H2):
        """uint8 frames [H,W,3] or [N,H,W,3] (numpy or tensor) -> uint8 [H2,W2,3] / [N,H2,W2,3] on the device, one launch on the current
        stream.  A refused geometry (``area_geometry_refused``) raises KeepHipError: there is no other path here."""
        W2, H2 = int(W2), int(H2)
        H, W = _frame_size(frames, 'resize_u8')
        x, batched = self._input(frames, 'resize_u8')
        if area_geometry_refused(H, W, H2, W2):
            raise L.KeepHipError(f"keep_resize_area_u8 refuses {W}x{H} -> {W2}x{H2}: INTER_AREA on the device is for shrinking on both "
                                 f"axes with a scale that is not a whole number on both", code=L.EINVAL)
        y = self._output(x, H2, W2, None, 'resize_u8')
        tables = self._device_tables(H, W, H2, W2) if len(x) else ()      # (an empty batch builds none)
        return self._launch('keep_resize_area_u8', x, y, batched, *tables)


class LinearResizer(_Resizer):
    """``cv2.resize(..., INTER_LINEAR)`` for uint8 3-channel frames; the kernel needs no tables, so there is nothing to cache.  One
    instance per processor."""

    def resize_u8(self, frames, W2, H2, out=None):
        """uint8 frames [H,W,3] or [N,H,W,3] (numpy or tensor) -> uint8 [H2,W2,3] / [N,H2,W2,3] on the device, one launch on the current
        stream.  At identity the input comes back as it is and nothing is launched, like ``Lanczos4Resizer.resize_u8``.  ``out``: a
        contiguous uint8 tensor of the result's shape on this device to write into (a slice of a larger batch) instead of a new one; at
        identity the frames are copied into it."""
        W2, H2 = int(W2), int(H2)
        H, W = _frame_size(frames, 'resize_u8')
        if (H, W) == (H2, W2) and out is None:
            return frames
        y = self._output(frames, H2, W2, out, 'resize_u8')
        if (H, W) == (H2, W2):
            return out.copy_(torch.as_tensor(frames), non_blocking=True)
        x, batched = self._input(frames, 'resize_u8')
        return self._launch('keep_resize_linear_u8', x, y, batched)

    @staticmethod
    def enlarged_size(H, W, fx, fy):
        """(W2, H2) of ``cv2.resize(img [H,W], (0, 0), fx=fx, fy=fy)``: ``saturate_cast<int>(S * f)`` per axis, i.e. round to nearest with
        ties to even -- Python's ``round``.  The one place that turns factors into a size."""
        return int(round(W * float(fx))), int(round(H * float(fy)))

    def enlarge_u8(self, frames, fx, fy, out=None):
        """``cv2.resize(frame, (0, 0), fx=fx, fy=fy, interpolation=INTER_LINEAR)`` over uint8 frames [H,W,3] or [N,H,W,3] (numpy or tensor)
        -> uint8 [H2,W2,3] / [N,H2,W2,3] on the device, one launch on the current stream; (W2, H2) = ``enlarged_size``.  Unlike
        ``resize_u8`` nothing is special at identity: the kernel's arithmetic copies.  ``out``: as in ``resize_u8``."""
        fx, fy = float(fx), float(fy)
        H, W = _frame_size(frames, 'enlarge_u8')
        if not (np.isfinite(fx) and np.isfinite(fy) and fx > 0 and fy > 0):
            raise ValueError(f"enlarge_u8: factors must be finite and positive, got fx={fx} fy={fy}")
        W2, H2 = self.enlarged_size(H, W, fx, fy)
        if H <= 0 or W <= 0 or H2 <= 0 or W2 <= 0:
            raise ValueError(f"enlarge_u8: empty source or destination ({W}x{H} -> {W2}x{H2})")
        y = self._output(frames, H2, W2, out, 'enlarge_u8')
        x, batched = self._input(frames, 'enlarge_u8')
        return self._launch('keep_resize_linear_fxy_u8', x, y, batched, fx, fy)
