"""Independent numpy restatement of OpenCV 4.x ``cv2.resize(src_u8, (W2, H2), interpolation=cv2.INTER_LINEAR)`` for 8-bit images of any
channel count and any geometry (modules/imgproc/src/resize.cpp).  Written from the description of that code, not from the kernel, so that
the tests do not compare the product with itself.  Two paths, as in cv2.resize:

  * ``H == 2 * H2 and W == 2 * W2``: INTER_LINEAR is replaced by INTER_AREA, whose 2 x 2 integer path averages each block,
    ``(a + b + c + d + 2) >> 2``;
  * everything else: resizeGeneric_ with HResizeLinear<uchar, int, short> and VResizeLinear<uchar, int, short, FixedPtCast<int, uchar,
    22>> -- per axis a source index and two 11-bit weights per destination index (``axis_coefficients``: Python floats are doubles, one
    rounding per operation), a horizontal pass in int32 and the vertical pass with its two intermediate shifts.
"""
import math

import numpy as np

WEIGHT_ONE = 2048        # INTER_RESIZE_COEF_SCALE = 1 << 11


def _sat_short(v):
    return max(-32768, min(32767, int(v)))


def axis_coefficients(S, D, is_column):
    """[(s, w0, w1)] for destination indices 0 .. D - 1 of an axis with S source pixels: the pixel pair is (s, s + 1), weights at scale
    2048.  Columns (``is_column``) outside [0, S - 1) are moved to the border pixel with weight (2048, 0); a row index stays as computed --
    ``resize_linear`` clamps the rows it reads -- and keeps its weights."""
    scale = 1.0 / (float(D) / float(S))
    out = []
    for d in range(D):
        f = np.float32((d + 0.5) * scale - 0.5)                  # product, then sum, each rounded to double; the cast rounds to float
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if is_column:
            if s < 0:
                s, f = 0, np.float32(0)
            if s >= S - 1:
                s, f = S - 1, np.float32(0)
        w0 = _sat_short(np.rint((np.float32(1) - f) * np.float32(WEIGHT_ONE)))
        w1 = _sat_short(np.rint(f * np.float32(WEIGHT_ONE)))
        out.append((s, w0, w1))
    return out


def is_half_size(H, W, H2, W2):
    return H == 2 * H2 and W == 2 * W2


def half_size_average(img):
    """The 2 x 2 integer path: every output value is the rounded mean of its block."""
    v = img.astype(np.int32)
    total = v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]
    return ((total + 2) >> 2).astype(np.uint8)


def resize_linear(img, W2, H2):
    """uint8 [H,W,C] -> uint8 [H2,W2,C]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, C = img.shape
    if is_half_size(H, W, H2, W2):
        return half_size_average(img)
    cols = axis_coefficients(W, W2, True)
    rows = axis_coefficients(H, H2, False)
    left = np.array([c[0] for c in cols])
    right = np.minimum(left + 1, W - 1)                           # (its weight is 0 wherever s + 1 is outside)
    a0 = np.array([c[1] for c in cols], np.int32)[:, None]
    a1 = np.array([c[2] for c in cols], np.int32)[:, None]
    v = img.astype(np.int32)
    out = np.empty((H2, W2, C), np.uint8)
    hcache = {}

    def horizontal(y):                                            # one source row through the horizontal pass: int32 [W2, C]
        y = min(max(y, 0), H - 1)
        if y not in hcache:
            hcache[y] = v[y, left] * a0 + v[y, right] * a1
        return hcache[y]
    for d, (s, b0, b1) in enumerate(rows):
        r0, r1 = horizontal(s), horizontal(s + 1)
        q = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
        out[d] = np.clip(q, 0, 255)
    return out
