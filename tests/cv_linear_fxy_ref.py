"""Independent numpy restatement of OpenCV 4.x ``cv2.resize(src_u8, (0, 0), fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR)`` -- the form
with an empty ``dsize`` that ``FaceRestoreHelper.read_image`` uses for frames whose short side is below 512
(face_restoration_helper.py:182-184).  Written from the description of modules/imgproc/src/resize.cpp, not from the kernel.  Against the
``dsize`` form (tests/cv_linear_ref.py):

  * the destination size is ``saturate_cast<int>(S * f)`` per axis: round to nearest, ties to even (``enlarged_size``);
  * the coordinate scale of an axis is ``1.0 / f`` ITSELF, not ``1.0 / (D / S)`` recomputed from the rounded size;
  * INTER_AREA's 2 x 2 path, which cv2.resize substitutes at a scale of exactly 2 on both axes, is not restated: ``read_image`` only
    enlarges, and the library refuses ``fx == fy == 0.5``.

Behind that it is resizeGeneric_ with HResizeLinear<uchar, int, short> and VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>>:
``(float)((d + 0.5) * scale - 0.5)``, floor, the column border rule and clamped rows, 11-bit weights, the horizontal pass in int32 and the
vertical pass with its two intermediate shifts.  Nothing is imported from tests/cv_linear_ref.py: its coefficient function derives the
scale from the sizes.
"""
import numpy as np

ONE = 1 << 11                      # INTER_RESIZE_COEF_SCALE


def enlarged_size(H, W, fx, fy):
    """(W2, H2): np.rint rounds half to even, as cvRound / saturate_cast<int>(double) do."""
    return int(np.rint(np.float64(W) * np.float64(fx))), int(np.rint(np.float64(H) * np.float64(fy)))


def coefficients(S, D, scale, is_column):
    """(s int64 [D], w0 int32 [D], w1 int32 [D]) of an axis with S source and D destination pixels at the GIVEN scale (a double)."""
    d = np.arange(D, dtype=np.float64)
    pos = ((d + 0.5) * np.float64(scale) - 0.5).astype(np.float32)      # product and difference in double, one cast to float
    s = np.floor(pos)
    frac = (pos - s).astype(np.float32)                                  # float - float
    s = s.astype(np.int64)
    if is_column:
        low, high = s < 0, s >= S - 1
        frac = np.where(low | high, np.float32(0), frac).astype(np.float32)
        s = np.where(low, 0, s)
        s = np.where(high, S - 1, s)
    w0 = np.clip(np.rint((np.float32(1) - frac) * np.float32(ONE)), -32768, 32767).astype(np.int32)
    w1 = np.clip(np.rint(frac * np.float32(ONE)), -32768, 32767).astype(np.int32)
    return s, w0, w1


def resize_linear_fxy(img, fx, fy):
    """uint8 [H,W,C] -> uint8 [H2,W2,C] with (W2, H2) = enlarged_size(H, W, fx, fy)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, _ = img.shape
    W2, H2 = enlarged_size(H, W, fx, fy)
    assert W2 > 0 and H2 > 0 and not (1.0 / fx == 2.0 and 1.0 / fy == 2.0)
    xs, a0, a1 = coefficients(W, W2, 1.0 / np.float64(fx), True)
    ys, b0, b1 = coefficients(H, H2, 1.0 / np.float64(fy), False)
    x1 = np.minimum(xs + 1, W - 1)                                       # (weight 0 wherever xs + 1 is outside)
    v = img.astype(np.int32)
    hor = v[:, xs] * a0[None, :, None] + v[:, x1] * a1[None, :, None]    # every source row through the horizontal pass: [H,W2,C]
    r0 = hor[np.clip(ys, 0, H - 1)] >> 4                                 # rows are clamped when read and keep their weights
    r1 = hor[np.clip(ys + 1, 0, H - 1)] >> 4
    q = (((b0[:, None, None] * r0) >> 16) + ((b1[:, None, None] * r1) >> 16) + 2) >> 2
    return np.clip(q, 0, 255).astype(np.uint8)
