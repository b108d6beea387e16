"""final_upscale_factor's Lanczos resize, host side (no GPU): the library's table builder (keep_lanczos4_tables, host C) against
the independent numpy restatement of OpenCV 4.x (tests/cv_lanczos_ref.py), the int32 headroom of the fixed-point passes, and the
restatement itself against cv2 where cv2 exists."""
import ctypes

import numpy as np
import pytest

import cv_lanczos_ref as R

SIZES = (1, 2, 3, 7, 360, 480, 512, 720, 1280, 1920)
FACTORS = tuple(k / 10 for k in range(5, 41))                  # the widget's range, 0.5 .. 4.0
EXTRA = ((300, 100), (9, 3), (1, 5))                             # whole-pixel source coordinates (the 1e30 branch); one source pixel


def geometries():
    g = {(S, int(S * f)) for S in SIZES for f in FACTORS if int(S * f) >= 1}
    return sorted(g | set(EXTRA))


def lib_tables(S, D):
    from comfyui_keep_amd.engine.resize import lanczos4_tables
    return lanczos4_tables(S, D)


def test_library_tables_equal_the_restatement():
    geo = geometries()
    assert len(geo) > 250
    for S, D in geo:
        ofs, coef = lib_tables(S, D)
        rofs, rcoef = R.axis_tables(S, D)
        assert ofs.dtype == np.int32 and coef.dtype == np.int16 and coef.shape == (D, 8)
        assert np.array_equal(ofs, rofs), (S, D)
        assert np.array_equal(coef, rcoef), (S, D, np.argwhere(coef != rcoef)[:4])


def test_whole_pixel_coordinates_take_the_centre_tap():
    """f == 0 (interpolateLanczos4's 1e30 branch): 300 -> 100 and 9 -> 3 sample source pixels 1, 4, 7, ... with the one-hot tap."""
    for S, D in ((300, 100), (9, 3)):
        ofs, coef = lib_tables(S, D)
        assert np.array_equal(ofs, 1 + 3 * np.arange(D))
        assert (coef == np.array([0, 0, 0, 2048, 0, 0, 0, 0], np.int16)).all()
    ofs, coef = lib_tables(1, 5)                       # one source pixel: every tap clamps to it, the weights still sum to ~2048
    assert (ofs >= -1).all() and (ofs <= 0).all() and (np.abs(coef.astype(int).sum(1) - 2048) <= 4).all()


def test_no_table_overflows_int32_in_the_vertical_pass():
    """h = sum_i u8 * ax[i] and v = sum_k h * ay[k] are int32 in the kernel (and in OpenCV): with the worst horizontal table of
    every geometry combined with the worst vertical one, v + 2^21 stays inside int32 for every uint8 input."""
    pos = neg = 0
    for S, D in geometries():
        c = lib_tables(S, D)[1].astype(np.int64)
        pos = max(pos, int(np.where(c > 0, c, 0).sum(1).max()))
        neg = min(neg, int(np.where(c < 0, c, 0).sum(1).min()))
    hmax, hmin = 255 * pos, 255 * neg
    vmax = hmax * pos + hmin * neg + (1 << 21)             # positive taps on the largest h, negative taps on the most negative h
    vmin = hmin * pos + hmax * neg
    assert vmax < 2 ** 31 and vmin >= -2 ** 31, (vmin, vmax)
    assert hmax < 2 ** 31 and hmin >= -2 ** 31


def test_bad_table_arguments_are_refused_without_a_device():
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_lanczos4_tables.restype = ctypes.c_int32
    lib.keep_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_int32 * 8)()
    assert lib.keep_lanczos4_tables(0, 4, buf, buf) == -1 and b'keep_lanczos4_tables' in lib.keep_last_error()
    assert lib.keep_lanczos4_tables(4, 4, None, buf) == -1
    with pytest.raises(hiplib.KeepHipError):
        lib_tables(5, 0)


def test_restatement_hand_cases():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    assert np.array_equal(R.resize_lanczos4(img, 17, 13), img)                      # identity is a copy
    for (h, w), (h2, w2) in (((13, 17), (26, 34)), ((40, 30), (20, 15)), ((9, 7), (31, 3)), ((5, 5), (1, 1))):
        for value in (0, 1, 128, 254, 255):
            flat = np.full((h, w, 3), value, np.uint8)
            assert (R.resize_lanczos4(flat, w2, h2) == value).all(), (value, h2, w2)   # a constant image stays constant
    # whole-pixel geometry: every output pixel is a source pixel (taps one-hot)
    big = rng.integers(0, 256, (9, 300, 3), dtype=np.uint8)
    assert np.array_equal(R.resize_lanczos4(big, 100, 3), big[1::3, 1::3])


def test_restatement_equals_opencv_where_opencv_exists():
    cv2 = pytest.importorskip('cv2')
    rng = np.random.default_rng(2)
    for S, D in geometries():
        if S > 720:
            continue
        h = 7 if S > 7 else S + 2
        img = rng.integers(0, 256, (h, S, 3), dtype=np.uint8)
        assert np.array_equal(R.resize_lanczos4(img, D, h), cv2.resize(img, (D, h), interpolation=cv2.INTER_LANCZOS4)), (S, D)
        img = rng.integers(0, 256, (S, 5, 3), dtype=np.uint8)
        assert np.array_equal(R.resize_lanczos4(img, 5, D), cv2.resize(img, (5, D), interpolation=cv2.INTER_LANCZOS4)), (S, D)
    img = rng.integers(0, 256, (360, 480, 3), dtype=np.uint8)
    for f in (0.5, 0.7, 1.3, 2.0, 4.0):
        w2, h2 = int(480 * f), int(360 * f)
        assert np.array_equal(R.resize_lanczos4(img, w2, h2), cv2.resize(img, (w2, h2), interpolation=cv2.INTER_LANCZOS4)), f
