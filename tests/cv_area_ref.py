"""Independent numpy restatement of OpenCV 4.x ``cv2.resize(src_u8x3, (W2, H2), interpolation=cv2.INTER_AREA)`` for frames that shrink
on both axes with a scale that is not a whole number on both (modules/imgproc/src/resize.cpp: computeResizeAreaTab,
ResizeArea_Invoker<uchar, float>).  Written from the description of that code, not from the library's table code, so that the tests do not
compare the product with itself.  Table arithmetic is Python float (double, one rounding per operation); the pixel loop is float32 numpy
element operations, multiply and add rounded separately.  ``fused=True`` emulates what a build with FMA contraction would compute
instead: product and sum in float64, rounded to float32 once (a uint8 x float32 and a float32 x float32 product are exact in float64).
"""
import math
import sys

import numpy as np


def axis_scale(S, D):
    return 1.0 / (float(D) / float(S))


def scale_is_whole(S, D):
    s = axis_scale(S, D)
    return abs(s - int(s)) < sys.float_info.epsilon


def is_area_fast(H, W, H2, W2):
    return scale_is_whole(H, H2) and scale_is_whole(W, W2)


def axis_entries(S, D):
    """[(di, si, alpha float32)] of one axis in OpenCV's order."""
    assert 0 < D < S
    scale = axis_scale(S, D)
    out = []
    for dx in range(D):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, S - fsx1)
        sx1, sx2 = math.ceil(fsx1), math.floor(fsx2)
        sx2 = min(sx2, S - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            out.append((dx, sx1 - 1, np.float32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            out.append((dx, sx, np.float32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            out.append((dx, sx2, np.float32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
    return out


def axis_csr(S, D):
    """(start int32 [D + 1], si int32 [n], alpha float32 [n]): the entries of destination d are start[d] .. start[d + 1]."""
    ent = axis_entries(S, D)
    start = np.zeros(D + 1, np.int32)
    for di, _, _ in ent:
        start[di + 1] += 1
    start = np.cumsum(start).astype(np.int32)
    assert [e[0] for e in ent] == sorted(e[0] for e in ent)
    return start, np.array([e[1] for e in ent], np.int32), np.array([e[2] for e in ent], np.float32)


def _mac(acc, a, b, fused):
    """acc + a * b on float32 arrays: two roundings, or one (through float64) when ``fused``."""
    if fused:
        return (acc.astype(np.float64) + a.astype(np.float64) * np.float64(b)).astype(np.float32)
    return (acc + (a * np.float32(b)).astype(np.float32)).astype(np.float32)


def resize_area(img, W2, H2, fused=False):
    """uint8 [H,W,3] -> uint8 [H2,W2,3]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W = img.shape[:2]
    assert H2 < H and W2 < W and not is_area_fast(H, W, H2, W2), "not the geometry of the general INTER_AREA path"
    xstart, xsi, xa = axis_csr(W, W2)
    ystart, ysi, ya = axis_csr(H, H2)
    src = img.astype(np.float32)
    # buf of every source row a y entry names: [H, W2, C], the x entries of a destination column in ascending order
    buf = np.zeros((H, W2, img.shape[2]), np.float32)
    for dx in range(W2):
        b = np.zeros((H, img.shape[2]), np.float32)
        for e in range(xstart[dx], xstart[dx + 1]):
            b = _mac(b, src[:, xsi[e]], xa[e], fused)
        buf[:, dx] = b
    out = np.empty((H2, W2, img.shape[2]), np.float32)
    for dy in range(H2):
        s = None
        for e in range(ystart[dy], ystart[dy + 1]):
            if s is None:
                s = (buf[ysi[e]] * np.float32(ya[e])).astype(np.float32)         # the first entry of a row: sum = beta * buf
            else:
                s = _mac(s, buf[ysi[e]], ya[e], fused)
        out[dy] = s
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)                           # cvRound (half to even), saturate_cast<uchar>
