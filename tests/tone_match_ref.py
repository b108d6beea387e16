"""The numpy restatement of the tone match (include/keep_cv_hip.h: keep_tone_match_u8; engine/tone.py), int64 throughout, with the bounds
the 16-bit / 32-bit operands of the kernel rest on asserted on the way.  Per channel, indices clamped at the borders:

    d  = src - rst
    hh = sum_k t[k] * d[y, clamp(x + k)]
    h4 = (hh + 128) >> 8                    |h4| <= 4080
    v  = sum_k t[k] * h4[clamp(y + k), x]   |v| < 2^31
    out = clamp(rst + ((v + 32768) >> 16), 0, 255)
"""
import numpy as np


def _filter_axis(a, taps, axis):
    """sum_k taps[k] * a[..., clamp(i + k), ...] along ``axis``, int64."""
    R = (len(taps) - 1) // 2
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k in range(-R, R + 1):
        idx = np.clip(np.arange(n) + k, 0, n - 1)
        out += int(taps[R + k]) * np.take(a, idx, axis=axis)
    return out


def tone_match_ref(src, rst, taps, with_bounds=False, with_clamped=False):
    """uint8 [F,h,w,3] (or [h,w,3]) source and restored images, the 2R + 1 integer taps -> the matched uint8 images of the same shape.
    ``with_bounds``: also (max |h4|, max |v|).  ``with_clamped``: also the number of outputs the final clamp changed."""
    src, rst = np.asarray(src), np.asarray(rst)
    assert src.dtype == np.uint8 and rst.dtype == np.uint8 and src.shape == rst.shape and src.shape[-1] == 3
    taps = np.asarray(taps).astype(np.int64)
    assert len(taps) % 2 == 1 and taps.min() >= 0 and int(taps.sum()) == 4096
    lead = src.ndim == 3
    s, r = (x[None] if lead else x for x in (src, rst))
    d = s.astype(np.int64) - r.astype(np.int64)
    hh = _filter_axis(d, taps, 2)
    h4 = (hh + 128) >> 8
    assert int(np.abs(h4).max()) <= 4080
    v = _filter_axis(h4, taps, 1)
    assert int(np.abs(v).max()) < 2 ** 31
    total = r.astype(np.int64) + ((v + 32768) >> 16)
    out = np.clip(total, 0, 255).astype(np.uint8)
    out = out[0] if lead else out
    if with_clamped:
        return out, int(((total < 0) | (total > 255)).sum())
    return (out, int(np.abs(h4).max()), int(np.abs(v).max())) if with_bounds else out
