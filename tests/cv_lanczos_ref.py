"""Independent numpy restatement of OpenCV 4.x ``cv2.resize(src_u8x3, (W2, H2), interpolation=cv2.INTER_LANCZOS4)``
(modules/imgproc/src/resize.cpp: resizeGeneric_, interpolateLanczos4, HResizeLanczos4<uchar,int,short,2048>,
VResizeLanczos4 with FixedPtCast<int,uchar,22>).  Written from the OpenCV source, not from the library's table code, so that the
tests do not compare the product with itself.  Every float / double operation is a separately rounded numpy element operation
(no FMA); sin / cos are the C library's (``math``), as in OpenCV's compiled code.
"""
import math

import numpy as np

_S45 = 0.70710678118654752440084436210485
_CS = np.array([[1, 0], [-_S45, -_S45], [0, 1], [_S45, -_S45], [-1, 0], [_S45, _S45], [0, -1], [-_S45, _S45]], np.float64)
_PI = 3.1415926535897932384626433832795


def axis_tables(S, D):
    """(ofs int64 [D], coef int16 [D, 8]) for source size S -> destination size D."""
    scale = 1.0 / (float(D) / float(S))
    d = np.arange(D, dtype=np.float64)
    fx = ((d + 0.5) * scale - 0.5).astype(np.float32)              # double multiply, double subtract, one rounding to float
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    x3 = (fx + np.float32(3.0)).astype(np.float32)                  # float add
    y0 = -x3.astype(np.float64) * _PI * 0.25
    s0 = np.array([math.sin(v) for v in y0], np.float64)
    c0 = np.array([math.cos(v) for v in y0], np.float64)
    coeffs = np.empty((D, 8), np.float32)
    total = np.zeros(D, np.float32)
    for i in range(8):
        yi = (x3 - np.float32(i)).astype(np.float32)
        y = -yi.astype(np.float64) * _PI * 0.25
        with np.errstate(divide='ignore', invalid='ignore'):
            ci = ((_CS[i, 0] * s0 + _CS[i, 1] * c0) / (y * y)).astype(np.float32)
        ci = np.where(np.abs(yi) >= np.float32(1e-6), ci, np.float32(1e30))
        coeffs[:, i] = ci
        total = (total + ci).astype(np.float32)                     # float sum, in tap order
    inv = (np.float32(1.0) / total).astype(np.float32)
    coeffs = (coeffs * inv[:, None]).astype(np.float32)
    fixed = np.rint((coeffs * np.float32(2048.0)).astype(np.float32))  # cvRound: half to even
    return sx, np.clip(fixed, -32768, 32767).astype(np.int16)


def tap_index(ofs, S):
    """[D, 8] source index of every tap: clamp(ofs - 3 + i, 0, S - 1)."""
    return np.clip(ofs[:, None] - 3 + np.arange(8)[None, :], 0, S - 1)


def int32_bounds(xcoef, ycoef):
    """(min, max) over all uint8 inputs of the vertical sum + 2^21 -- what must fit int32 for the fixed-point passes."""
    xc, yc = xcoef.astype(np.int64), ycoef.astype(np.int64)
    hmax = 255 * np.where(xc > 0, xc, 0).sum(1).max()
    hmin = 255 * np.where(xc < 0, xc, 0).sum(1).min()
    vmax = np.where(yc > 0, yc * hmax, yc * hmin).sum(1).max()
    vmin = np.where(yc > 0, yc * hmin, yc * hmax).sum(1).min()
    hlo = min(hmin, 0)
    return int(min(vmin, hlo)), int(max(vmax, hmax) + (1 << 21))


def resize_lanczos4(img, W2, H2):
    """uint8 [H,W,3] (or [H,W]) -> uint8 [H2,W2,3]: the tables above, exact integer sums, (v + 2^21) >> 22 clamped."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    H, W = img.shape[:2]
    if (H, W) == (H2, W2):
        return img.copy()
    xo, xc = axis_tables(W, W2)
    yo, yc = axis_tables(H, H2)
    src = img.astype(np.int64)
    cols, rows = tap_index(xo, W), tap_index(yo, H)
    xw = xc.astype(np.int64) if img.ndim == 2 else xc.astype(np.int64)[:, :, None]
    h = sum(src[:, cols[:, i]] * xw[:, i] for i in range(8))                         # [H, W2(, 3)]
    yw = yc.astype(np.int64).reshape((H2, 8) + (1,) * (img.ndim - 1))
    v = sum(h[rows[:, k]] * yw[:, k] for k in range(8))                              # [H2, W2(, 3)]
    assert v.min() >= -(1 << 31) and v.max() + (1 << 21) < (1 << 31)
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
