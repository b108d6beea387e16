"""Alias-free paste-back (KEEP_AMD_PASTE_AA), host side (no GPU): the rule (engine/paste.py: ``aa_factor``, ``ss_affine``), the numpy
restatement tests/paste_aa_ref.py -- its reduction to tests/paste_fade_ref.py at N = 1 and the checkerboard property the mode exists for
--, the entry point keep_paste_face_aa in header, binding and library with the launcher's refusals (host checks), and the processor's
knob over a fake paster.

The checkerboard property: a one-pixel checkerboard face (0 / 255) pasted at scale r < 1 is a flat 127.5 to a filter that covers the frame
pixel's footprint, and whatever phase the taps hit to a filter one crop pixel wide.  Over the pixels where both soft masks exceed 0.999
the default spans 0 .. 255 with std > 30, the area-sampled output stays within 127.5 +- 14 with std < 5.  Measured on the restatement
(160 x 200 frame): r = 0.25 at 0.2 rad 121 .. 134 (std 2.7; default std 42.5), r = 0.2 at 0.1 rad 125 .. 130, r = 0.6 at 0.15 rad
114 .. 140."""
import ctypes
import logging
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import paste_aa_ref as AR
import paste_fade_ref as FR
import paste_oracle as P

NAME = 'keep_paste_face_aa'
CHECKER = [(0.25, 0.2), (0.2, 0.1), (0.6, 0.15)]


def paste():
    from comfyui_keep_amd.engine import paste
    return paste


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def test_aa_factor_on_both_sides_of_every_threshold():
    f = paste().aa_factor
    up, dn = math.nextafter, math.nextafter
    for theta in (0.0, 0.3, -1.2):
        M = lambda r: AR.similarity(r, theta, 12.5, -3.25)                                # noqa: E731
        assert f(M(3.0)) == 1 and f(M(1.18)) == 1 and f(M(1.001)) == 1
        assert f(M(0.999)) == 2 and f(M(0.74)) == 2 and f(M(0.501)) == 2
        assert f(M(0.499)) == 4 and f(M(0.39)) == 4 and f(M(0.251)) == 4
        assert f(M(0.249)) == 8 and f(M(0.176)) == 8 and f(M(0.05)) == 8
    # exactly on a threshold (axis-aligned: the determinant is r * r, exact for these powers of two)
    diag = lambda r: np.array([[r, 0, 0], [0, r, 0]], np.float64)                         # noqa: E731
    assert [f(diag(r)) for r in (1.0, 0.5, 0.25, 0.125)] == [1, 2, 4, 8]
    assert f(diag(dn(1.0, 0.0))) == 2 and f(diag(dn(0.5, 0.0))) == 4 and f(diag(dn(0.25, 0.0))) == 8 and f(diag(up(0.5, 1.0))) == 2
    # a reflection counts by |det|; a singular or non-finite matrix takes today's tap
    assert f(np.array([[0.3, 0, 0], [0, -0.3, 0]])) == 4
    assert f(np.zeros((2, 3))) == 1 and f(np.array([[1.0, 2.0, 5.0], [0.5, 1.0, 7.0]])) == 1
    assert f(np.array([[np.nan, 0, 0], [0, 0.3, 0]])) == 1 and f(np.array([[np.inf, 0, 0], [0, 0.3, 0]])) == 1
    assert f(np.array([[0.3, 0, 0], [0, 0.3, 0]], np.float32)) == 4 and f([[0.3, 0, 0], [0, 0.3, 0]]) == 4


def test_ss_affine_of_one_is_the_matrix_bit_for_bit():
    ss = paste().ss_affine
    M = np.array([[0.1757, -0.0176, -0.0], [0.0176, 0.1757, 50.7]], np.float64)             # (-0.0 + 0.0 would lose its sign)
    got = ss(M, 1)
    assert got.dtype == np.float64 and got.tobytes() == M.tobytes() and got is not M
    assert np.array_equal(ss(M, 4), [[4 * M[0, 0], 4 * M[0, 1], 4 * M[0, 2] + 1.5], [4 * M[1, 0], 4 * M[1, 1], 4 * M[1, 2] + 1.5]])


@pytest.mark.parametrize('N', [2, 4, 8])
def test_sub_sample_positions_follow_the_offset_formula(N):
    """Pixel (N x + i, N y + j) of the fine grid is the point of the frame at (x, y) + ((2 i + 1 - N) / 2 N, (2 j + 1 - N) / 2 N): the
    inverse of ss_affine there is the inverse of M at that point, and the N x N offsets tile the pixel's square [-1/2, 1/2)^2 evenly."""
    mod = paste()
    M = AR.similarity(0.39, 0.2, 40.3, 50.7)
    inv, inv_fine = mod.invert_affine(M), mod.invert_affine(mod.ss_affine(M, N))
    offs = [(2 * i + 1 - N) / (2 * N) for i in range(N)]
    assert offs[0] == -(N - 1) / (2 * N) and offs[-1] == (N - 1) / (2 * N) and np.allclose(np.diff(offs), 1 / N) and abs(sum(offs)) < 1e-12
    for x, y in ((0, 0), (17, 5), (199, 159)):
        for j in range(N):
            for i in range(N):
                fine = inv_fine @ np.array([N * x + i, N * y + j, 1.0])
                want = inv @ np.array([x + offs[i], y + offs[j], 1.0])
                assert np.allclose(fine, want, rtol=0, atol=1e-9), (x, y, i, j)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_restatement_at_one_sub_sample_is_the_weighted_restatement():
    frame, faces, mats, classes = FR.small_case()
    assert [paste().aa_factor(M) for M in mats] == [8, 8]
    for cls in (list(classes), None):
        for weights in (None, [0.5, float(np.float32(1.0 / 3.0))]):
            want = FR.paste_faces_weighted(frame, list(faces), list(mats), cls, weights=weights)
            got = AR.paste_faces_aa(frame, list(faces), list(mats), cls, weights=weights, factors=[1, 1])
            assert (want != frame).any() and got.dtype == np.uint8 and np.array_equal(got, want)
    # a face that is not shrunk takes N = 1 by the rule itself
    big = [AR.similarity(1.18, 0.1, -200.0, -150.0), None]
    assert paste().aa_factor(big[0]) == 1
    want = FR.paste_faces_weighted(frame, list(faces), big, list(classes))
    assert (want != frame).any() and np.array_equal(AR.paste_faces_aa(frame, list(faces), big, list(classes)), want)


@pytest.fixture(scope='module')
def all_skin():
    return P.parse_soft_mask(np.ones((512, 512), np.uint8))


@pytest.mark.parametrize('r,theta', CHECKER)
def test_checkerboard_property_on_the_restatement(all_skin, r, theta):
    frame, face, M, cls = AR.checkerboard_case(r, theta)
    N = paste().aa_factor(M)
    assert N == {0.25: 4, 0.2: 8, 0.6: 2}[r]
    soft1 = AR.frame_soft_masks(frame, [face], [M], [cls], factors=[1], parse_soft=[all_skin])
    softn = AR.frame_soft_masks(frame, [face], [M], [cls], parse_soft=[all_skin])
    default = AR.paste_faces_aa(frame, [face], [M], [cls], factors=[1], soft=soft1)
    assert np.array_equal(default, P.paste_faces(frame, [face], [M], [cls]))            # the default IS the reference arithmetic
    aa = AR.paste_faces_aa(frame, [face], [M], [cls], soft=softn)
    sel = (soft1[0] > 0.999) & (softn[0] > 0.999)
    d, a = default[sel].astype(np.float64), aa[sel].astype(np.float64)
    print(f"r {r} theta {theta} N {N}: {int(sel.sum())} pixels; default {d.min():.0f} .. {d.max():.0f} std {d.std():.2f}; "
          f"area-sampled {a.min():.0f} .. {a.max():.0f} std {a.std():.2f}")
    assert sel.sum() > 5000
    assert d.min() == 0 and d.max() == 255 and d.std() > 30
    assert a.min() >= 127.5 - 14 and a.max() <= 127.5 + 14 and a.std() < 5
    zero = softn[0] == 0
    if r < 0.6:                                       # (at r = 0.6 the face covers the whole frame)
        assert zero.sum() > 1000
    assert np.array_equal(aa[zero], frame[zero])


def test_axis_aligned_checkerboard_collapses_to_the_phase_the_taps_hit(all_skin):
    """r = 0.25 without rotation: every tap of the default lands on one parity of the board -- a flat 0 --, the area-sampled form gives
    its mean."""
    frame, face, M, cls = AR.checkerboard_case(0.25, 0.0)
    soft1 = AR.frame_soft_masks(frame, [face], [M], [cls], factors=[1], parse_soft=[all_skin])
    softn = AR.frame_soft_masks(frame, [face], [M], [cls], parse_soft=[all_skin])
    sel = (soft1[0] > 0.999) & (softn[0] > 0.999)
    default = AR.paste_faces_aa(frame, [face], [M], [cls], factors=[1], soft=soft1)[sel]
    aa = AR.paste_faces_aa(frame, [face], [M], [cls], soft=softn)[sel]
    assert sel.sum() > 5000 and default.min() == default.max() == 0 and 127 <= aa.min() and aa.max() <= 128


# ---- the entry point ----------------------------------------------------------------------------------------------------------------------
def raw_lib():
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_last_error.restype = ctypes.c_char_p
    return lib


def test_symbol_is_in_the_extension_header_the_binding_and_the_library_only():
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    core = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    assert re.search(r'int32_t ' + NAME + r'\s*\(', header) and NAME not in core
    assert '#define KEEP_CV_ABI_VERSION 1' in header and hiplib.CV_ABI_VERSION == 1        # one more symbol, the same version
    assert NAME in hiplib.CV_EXPORTED_SYMBOLS and NAME in hiplib._CV_SIGNATURES
    assert NAME not in hiplib.EXPORTED_SYMBOLS and NAME not in hiplib._SIGNATURES
    assert hasattr(raw_lib(), NAME)
    proto = re.search(r'int32_t ' + NAME + r'\s*\(([^;]*)\);', header).group(1)
    assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == len(hiplib._CV_SIGNATURES[NAME]) == 16
    # keep_paste_face_w's argument list with n in front of the opacity
    w_sig = hiplib._CV_SIGNATURES['keep_paste_face_w']
    assert hiplib._CV_SIGNATURES[NAME] == w_sig[:-2] + [ctypes.c_int32] + w_sig[-2:]
    bound = hiplib.load(check_device=False)
    assert getattr(bound, NAME).argtypes == hiplib._CV_SIGNATURES[NAME] and getattr(bound, NAME).restype is ctypes.c_int32


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """A bad n -- and everything keep_paste_face_w refuses -- is refused with KEEP_EINVAL before anything is launched, on a machine
    without a GPU: the device pointers (placeholders here) are never dereferenced."""
    lib = raw_lib()
    f = getattr(lib, NAME)
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                  ctypes.c_void_p] + [ctypes.c_int32] * 6 + [ctypes.c_float, ctypes.c_void_p]
    d2s = (ctypes.c_double * 6)(1, 0, 0, 0, 1, 0)

    def call(frame=0x1000, H=200, W=300, face=0x2000, mask=0x3000, fh=512, fw=512, m=d2s, box=(50, 50, 50, 90), border=10, n=4, opacity=0.5):
        return f(frame, H, W, face, mask, fh, fw, m, *box, border, n, opacity, None)
    refused = [dict(n=0), dict(n=1), dict(n=3), dict(n=5), dict(n=6), dict(n=16), dict(n=-2), dict(opacity=-0.25), dict(opacity=1.5),
               dict(opacity=float('nan')), dict(opacity=float('inf')), dict(opacity=1.0000001), dict(frame=None), dict(face=None),
               dict(mask=None), dict(m=None), dict(H=0), dict(fw=1), dict(box=(-1, 10, 100, 100)), dict(box=(10, 10, 301, 100)),
               dict(box=(10, 10, 100, 201))]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(NAME.encode() + b':'), (kw, lib.keep_last_error())
    for n in (2, 4, 8):                                                                       # an empty box launches nothing
        assert call(n=n) == 0 and call(n=n, box=(50, 50, 40, 90), opacity=0.0) == 0 and call(n=n, border=-1) == 0


# ---- the processor over a fake paster -------------------------------------------------------------------------------------------------------
class _FakePaster:
    """Records what ``GpuPaster.paste`` is handed; reports the rule's N per face like the real one."""

    def __init__(self):
        self.calls, self.last_aa = [], None

    def paste(self, bg, faces, mats, classes, factor, draw_box, **kw):
        self.calls.append(dict(kw))
        self.last_aa = [None if M is None else paste().aa_factor(M) for M in mats] if kw.get('aa') else None
        return torch.as_tensor(bg).clone()


class _PasteHelper:
    use_parse, face_parse, upscale_factor, face_size = False, None, 1, (512, 512)

    def __init__(self, mats):
        self.input_img = np.zeros((64, 80, 3), np.uint8)
        self.restored_faces = [np.zeros((512, 512, 3), np.uint8) for _ in mats]
        self.inverse_affine_matrices = list(mats)
        self.own = 0

    def paste_faces_to_input_image(self, upsample_img=None, draw_box=False, face_upsampler=None):
        self.own += 1
        return upsample_img


def _paste_processor():
    from test_host_logic import _pack, _U8Net
    from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor
    proc = KEEPFaceProcessor(_pack(_U8Net(True)))
    proc.device = 'cpu'
    proc.gpu_paste, proc._gpu_paste_forced = True, True            # the erosion-mask composite: no ParseNet in front of the paster
    proc._paster = _FakePaster()
    return proc


def test_processor_knob_reaches_the_paster_only_when_on(monkeypatch):
    from test_host_logic import _pack, _U8Net
    from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor
    monkeypatch.delenv('KEEP_AMD_PASTE_AA', raising=False)
    assert KEEPFaceProcessor(_pack(_U8Net(True))).paste_aa is False
    monkeypatch.setenv('KEEP_AMD_PASTE_AA', '0')
    assert KEEPFaceProcessor(_pack(_U8Net(True))).paste_aa is False
    monkeypatch.setenv('KEEP_AMD_PASTE_AA', '1')
    assert KEEPFaceProcessor(_pack(_U8Net(True))).paste_aa is True
    monkeypatch.delenv('KEEP_AMD_PASTE_AA')
    mats = [AR.similarity(0.39, 0.1, 5.0, 5.0), AR.similarity(1.18, 0.0, 0.0, 0.0), AR.similarity(0.1, 0.0, 30.0, 30.0),
            AR.similarity(0.3, 0.2, 9.0, 9.0)]
    bg = np.zeros((64, 80, 3), np.uint8)
    proc = _paste_processor()
    helper = _PasteHelper(mats)
    # off: today's call, argument for argument -- with and without a fade
    proc._paste(helper, bg, False)
    proc._paste(helper, bg, False, weights=[1.0, 0.5, 1.0, 1.0])
    assert proc._paster.calls == [{}, {'weights': [1.0, 0.5, 1.0, 1.0]}] and not hasattr(proc, 'last_paste_aa') and helper.own == 0
    # on
    proc.paste_aa = True
    proc._paster.calls.clear()
    proc._aa_begin()
    proc._paste(helper, bg, False)
    assert proc._paster.calls == [{'aa': True}] and proc.last_paste_aa == {4: 2, 1: 1, 8: 1}
    proc._paste(helper, bg, False, weights=[1.0, 0.5, 1.0, 1.0])
    assert proc._paster.calls[1] == {'weights': [1.0, 0.5, 1.0, 1.0], 'aa': True} and proc.last_paste_aa == {4: 4, 1: 2, 8: 2}
    proc._aa_begin()                                                # the next public call counts from nothing
    assert proc.last_paste_aa == {}


def test_the_helpers_own_paste_ignores_the_knob_with_one_warning():
    from test_clip_plan_host import _MarkNet, _frames, _processor
    records = []

    class Catch(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())
    handler = Catch()
    logging.getLogger('ComfyUI-KEEP').addHandler(handler)
    try:
        off = _processor(_MarkNet(True), 1, False)                  # (gpu_paste False: the helper's own warp and paste)
        want = off.process_frames_u8(_frames(5), 1.0, False, False, False, max_clip_length=4)
        assert not records
        on = _processor(_MarkNet(True), 1, False)
        on.paste_aa = True
        for _ in range(2):
            got = on.process_frames_u8(_frames(5), 1.0, False, False, False, max_clip_length=4)
            assert len(got) == 5 and all(np.array_equal(a, b) for a, b in zip(got, want))
        assert on.last_paste_aa == {}
        img = on.process_image(_frames(1)[0], 1.0, False, False, False)
        assert img is not None
    finally:
        logging.getLogger('ComfyUI-KEEP').removeHandler(handler)
    assert sum('KEEP_AMD_PASTE_AA' in m for m in records) == 1 and len(records) == 1
