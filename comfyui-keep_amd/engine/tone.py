"""Tone match of restored faces on the MI355X (csrc/keep_tone.hip, ``keep_tone_match_u8``): the restored face keeps its high spatial band
and takes the low band -- lighting, skin tone, white balance -- of the crop it was made from,

    out = restored - lowpass(restored) + lowpass(source) = restored + lowpass(source - restored)

with one separable Gaussian of the difference image, in integers throughout (include/keep_cv_hip.h spells the arithmetic out;
tests/tone_match_ref.py restates it in numpy).  The result is bit-reproducible: it depends neither on the batch nor on the launch geometry.

``tone_taps`` is pure numpy and needs no GPU.  No reference to compare with: the reference project has nothing like it.
"""
import ctypes as C
import math

import numpy as np

TAP_SUM = 4096          # the taps are 12-bit fixed point
R_MAX = 128             # the kernel's limit on the radius: sigma up to 128 / 3
FACES_PER_LAUNCH = 32   # the int16 intermediate of a launch (1.5 MB per 512 x 512 face) stays in the Infinity Cache


def tone_radius(sigma):
    """``R = ceil(3 sigma)``; ValueError for a sigma with 3 sigma outside 1 .. 128 (sigma roughly [0.34, 42.6]) or that is not a number."""
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"tone match: sigma must be a number, got {sigma!r}")
    if not math.isfinite(sigma) or sigma <= 0:
        raise ValueError(f"tone match: sigma must be positive and finite, got {sigma}")
    if not 1.0 <= 3.0 * sigma <= R_MAX:        # (a Gaussian that ends inside the first pixel is no low-pass; 128 is the kernel's limit)
        raise ValueError(f"tone match: sigma {sigma} puts 3 sigma outside 1 .. {R_MAX} pixels (sigma roughly 0.34 .. 42.6)")
    return int(math.ceil(3.0 * sigma))


def tone_taps(sigma):
    """The 2R + 1 integer taps of the low-pass, int16: g[k] = exp(-k^2 / (2 sigma^2)) in float64 for k = -R .. R, t = rint(g / sum(g) * 4096),
    and the centre tap takes what the rounding left of 4096.  Non-negative, symmetric, sum exactly 4096."""
    R = tone_radius(sigma)
    sigma = float(sigma)
    k = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    t = np.rint(g / g.sum() * TAP_SUM).astype(np.int64)
    t[R] += TAP_SUM - int(t.sum())
    if t.min() < 0 or int(t.sum()) != TAP_SUM or not np.array_equal(t, t[::-1]):
        raise ValueError(f"tone match: sigma {sigma} has no admissible taps")       # (no sigma of the admissible range gets here)
    return t.astype(np.int16)


class ToneMatcher:
    """One per processor, like ``GpuPaster``: the taps per sigma and one scratch buffer per launch shape are cached."""

    def __init__(self, device='cuda'):
        import torch
        from . import hiplib as L
        self._torch, self._L = torch, L
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        L.load()
        self._taps = {}
        self._scratch = {}

    def _taps_for(self, sigma):
        key = float(sigma)
        hit = self._taps.get(key)
        if hit is None:
            t = tone_taps(key)
            hit = self._taps[key] = ((C.c_int16 * len(t))(*t.tolist()), (len(t) - 1) // 2)
        return hit

    def _as_device(self, x, name):
        torch = self._torch
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        elif not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f) for f in x])))
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"ToneMatcher.match: {name} must be uint8 [F,h,w,3], got {x.dtype} {tuple(x.shape)}")
        return x.to(self.device, non_blocking=True).contiguous()

    def match(self, src_u8, rst_u8, sigma):
        """uint8 [F,h,w,3] source crops and restored faces (device tensors, or numpy arrays / lists of them, which are uploaded) -> the
        matched faces, a NEW uint8 [F,h,w,3] device tensor.  At most 32 faces per launch, on the current stream."""
        torch, L = self._torch, self._L
        taps, R = self._taps_for(sigma)
        src, rst = self._as_device(src_u8, 'src'), self._as_device(rst_u8, 'rst')
        if src.shape != rst.shape:
            raise ValueError(f"ToneMatcher.match: src {tuple(src.shape)} and rst {tuple(rst.shape)} differ")
        F, h, w, _ = src.shape
        with torch.cuda.device(self.device):
            out = torch.empty_like(rst)
            if F == 0:
                return out
            m = min(F, FACES_PER_LAUNCH)
            scratch = self._scratch.get((h, w))             # one buffer per face shape, as many faces as the largest launch so far
            if scratch is None or scratch.shape[0] < m:
                if scratch is not None:
                    scratch.record_stream(torch.cuda.current_stream())
                scratch = self._scratch[(h, w)] = torch.empty((m, h, w, 3), dtype=torch.int16, device=self.device)
            for a in range(0, F, FACES_PER_LAUNCH):
                b = min(F, a + FACES_PER_LAUNCH)
                L.call('keep_tone_match_u8', src[a:b], rst[a:b], out[a:b], scratch, b - a, h, w, taps, R)
        return out
