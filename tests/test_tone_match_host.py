"""Tone match of restored faces (engine/tone.py, keep_tone_match_u8), host side (no GPU): the taps (engine/tone.py:tone_taps), the properties of the arithmetic on its numpy
restatement (tests/tone_match_ref.py), the new entry point keep_tone_match_u8 -- header, binding, library, Makefile and the launcher's
refusals, which are host checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tone_match_ref import tone_match_ref

from comfyui_keep_amd.engine import tone as T

NAME = 'keep_tone_match_u8'
SIGMAS = [0.34, 0.5, 1, 4, 16, 40, 42.6]


# ---- the taps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', SIGMAS)
def test_taps_are_non_negative_symmetric_and_sum_to_4096(sigma):
    t = T.tone_taps(sigma)
    R = math.ceil(3 * sigma)
    assert t.dtype == np.int16 and len(t) == 2 * R + 1 and 1 <= R <= 128
    assert int(t.astype(np.int64).sum()) == 4096 and int(t.min()) >= 0 and np.array_equal(t, t[::-1])
    assert int(t[R]) == int(t.max())


def test_taps_the_table_of_the_definition():
    table = {1: (3, 1636, 7), 4: (12, 408, 25), 16: (48, 108, 97)}
    for sigma, (R, centre, positive) in table.items():
        t = T.tone_taps(sigma)
        assert ((len(t) - 1) // 2, int(t[R]), int((t > 0).sum())) == (R, centre, positive), sigma
    t = T.tone_taps(40)
    assert len(t) == 241 and int(t[120]) == 42 and int((t == 0).sum()) > 0              # some tail taps round to 0
    # the definition, spelt out once more
    k = np.arange(-12, 13, dtype=np.float64)
    g = np.exp(-k * k / 32.0)
    want = np.rint(g / g.sum() * 4096).astype(np.int64)
    want[12] += 4096 - want.sum()
    assert np.array_equal(T.tone_taps(4), want)


@pytest.mark.parametrize('sigma', [0.3, 43, 0, -1, float('nan'), float('inf'), 'x'])
def test_a_sigma_outside_the_admissible_range_raises(sigma):
    with pytest.raises(ValueError, match='tone match'):
        T.tone_taps(sigma)


# ---- the arithmetic, on the restatement -----------------------------------------------------------------------------------------------
SHAPES = [(5, 7), (33, 65), (128, 128)]


@pytest.mark.parametrize('hw', SHAPES, ids=lambda s: '%dx%d' % s)
def test_identity_and_constant_shift(hw):
    h, w = hw
    rst = np.random.default_rng(h).integers(40, 200, (2, h, w, 3), dtype=np.uint8)
    for sigma in (1, 16):
        taps = T.tone_taps(sigma)
        assert np.array_equal(tone_match_ref(rst, rst, taps), rst)
        for c in (-37, -1, 1, 40):
            src = (rst.astype(np.int64) + c).astype(np.uint8)
            assert np.array_equal(tone_match_ref(src, rst, taps), src), (sigma, c)


def test_the_extremes():
    hi, lo = np.full((1, 64, 64, 3), 255, np.uint8), np.zeros((1, 64, 64, 3), np.uint8)
    for sigma in (0.5, 16, 42.6):
        taps = T.tone_taps(sigma)
        out, h4, v = tone_match_ref(hi, lo, taps, with_bounds=True)
        assert (out == 255).all() and h4 == 4080 and v == 4080 * 4096 < 2 ** 24
        assert (tone_match_ref(lo, hi, taps) == 0).all()


@pytest.mark.parametrize('sigma', [0.34, 4, 42.6])
def test_the_bounds_hold_on_full_range_noise(sigma):
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (2, 33, 65, 3), dtype=np.uint8)
    rst = rng.integers(0, 256, (2, 33, 65, 3), dtype=np.uint8)
    out, h4, v = tone_match_ref(src, rst, T.tone_taps(sigma), with_bounds=True)     # (the asserts inside are the test)
    assert out.dtype == np.uint8 and out.shape == src.shape and h4 <= 4080 and v < 2 ** 24
    assert np.array_equal(tone_match_ref(src[1], rst[1], T.tone_taps(sigma)), out[1])  # a face does not depend on its batch


def test_the_restatement_is_the_definition_pixel_by_pixel():
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, (4, 6, 3), dtype=np.uint8)
    rst = rng.integers(0, 256, (4, 6, 3), dtype=np.uint8)
    t = [int(v) for v in T.tone_taps(1)]
    R, h, w = 3, 4, 6
    d = src.astype(int) - rst.astype(int)
    want = np.zeros_like(rst)
    for c in range(3):
        h4 = [[(sum(t[k + R] * int(d[y, min(max(x + k, 0), w - 1), c]) for k in range(-R, R + 1)) + 128) >> 8 for x in range(w)] for y in range(h)]
        for y in range(h):
            for x in range(w):
                v = sum(t[k + R] * h4[min(max(y + k, 0), h - 1)][x] for k in range(-R, R + 1))
                want[y, x, c] = min(max(int(rst[y, x, c]) + ((v + 32768) >> 16), 0), 255)
    assert np.array_equal(tone_match_ref(src, rst, t), want)


# ---- the entry point --------------------------------------------------------------------------------------------------------------------
def raw_lib():
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_last_error.restype = ctypes.c_char_p
    return lib


def test_symbol_is_in_the_extension_header_the_binding_the_library_and_the_makefile_only():
    """(The declaration has ten parameters -- src, rst, out, scratch, F, h, w, taps, R, stream -- and so has the binding.)"""
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    core = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    assert re.search(r'int32_t ' + NAME + r'\s*\(', header) and NAME not in core and 'tone' not in core
    assert NAME in hiplib.CV_EXPORTED_SYMBOLS and NAME in hiplib._CV_SIGNATURES
    assert NAME not in hiplib.EXPORTED_SYMBOLS and NAME not in hiplib._SIGNATURES and len(hiplib.EXPORTED_SYMBOLS) == 63
    assert hasattr(raw_lib(), NAME)
    proto = re.search(r'int32_t ' + NAME + r'\s*\(([^;]*)\);', header).group(1)
    assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == len(hiplib._CV_SIGNATURES[NAME]) == 10
    assert int(re.search(r'#define KEEP_CV_ABI_VERSION (\d+)', header).group(1)) == hiplib.CV_ABI_VERSION == 1
    bound = hiplib.load(check_device=False)
    assert getattr(bound, NAME).argtypes == hiplib._CV_SIGNATURES[NAME] and getattr(bound, NAME).restype is ctypes.c_int32
    assert 'keep_tone.hip' in open(os.path.join(ROOT, 'comfyui-keep_amd', 'csrc', 'Makefile')).read()
    assert NAME in open(os.path.join(ROOT, 'comfyui-keep_amd', 'csrc', 'keep_tone.hip')).read()


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """Every bad argument is refused with KEEP_EINVAL on a machine without a GPU: the checks run on the host before the first launch, and
    the device pointers (placeholders here) are never dereferenced."""
    lib = raw_lib()
    f = getattr(lib, NAME)
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int32] * 3 + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    good = [int(v) for v in T.tone_taps(1)]                     # R = 3
    n = 2 * 5 * 7 * 3                                           # bytes of src / rst / out; the scratch has 2 n

    def call(src=0x100000, rst=0x200000, out=0x300000, scratch=0x400000, F=2, h=5, w=7, taps=good, R=3):
        arr = None if taps is None else (ctypes.c_int16 * len(taps))(*taps)
        return f(src, rst, out, scratch, F, h, w, arr, R, None)
    neg = list(good)
    neg[0], neg[3] = -1, good[3] + good[0] + 1                  # still sums to 4096
    less, more = list(good), list(good)
    less[3] -= 1
    more[3] += 1
    refused = [dict(src=None), dict(rst=None), dict(out=None), dict(scratch=None), dict(taps=None),
               dict(F=0), dict(F=-1), dict(h=0), dict(h=-3), dict(w=0), dict(w=-1), dict(h=32768), dict(w=32768), dict(w=2 ** 31 - 1),
               dict(R=0), dict(R=129), dict(R=-1), dict(taps=neg), dict(taps=less), dict(taps=more),
               dict(out=0x200000), dict(out=0x100000), dict(scratch=0x100000), dict(scratch=0x200000), dict(scratch=0x300000),
               dict(out=0x200000 + 16), dict(out=0x200000 - n + 1), dict(scratch=0x300000 - 2 * n + 1), dict(out=0x400000 + 2 * n - 1)]
    assert sum(neg) == 4096 and sum(less) == 4095 and sum(more) == 4097
    for kw in refused:
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(NAME.encode() + b':'), (kw, lib.keep_last_error())
