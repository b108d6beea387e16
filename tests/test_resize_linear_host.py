"""The aligned-input resize (cv2.resize INTER_LINEAR restated: csrc/keep_resize_linear.hip, include/keep_cv_hip.h), host side (no GPU):
the independent numpy restatement (tests/cv_linear_ref.py) against the oracle's and against properties of the arithmetic, the extension
header against the binding and the built library, the launcher's refusals, and the processor's choice of who resizes."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import cv_linear_ref as R
from conftest import ROOT

# (H, W) -> (H2, W2), none an exact 2x shrink on both axes
GENERAL = [((23, 31), (64, 64)), ((90, 120), (64, 64)), ((130, 96), (64, 48)), ((60, 80), (7, 9)), ((1, 9), (4, 20)), ((9, 1), (20, 4)),
           ((5, 7), (1, 1)), ((37, 53), (37, 80)), ((64, 64), (128, 128))]


def image(h, w, c=3, seed=None):
    return np.random.default_rng(h * 1000 + w if seed is None else seed).integers(0, 256, (h, w, c), dtype=np.uint8)


@pytest.mark.parametrize('hw,hw2', GENERAL)
def test_restatement_equals_the_oracle_on_general_geometries(hw, hw2):
    import facelib_oracle as FO
    img = image(*hw)
    assert np.array_equal(R.resize_linear(img, hw2[1], hw2[0]), FO.cv2_resize_linear_u8(img, hw2[1], hw2[0]))


def test_identity_is_a_copy_and_constant_frames_stay_constant():
    img = image(19, 27)
    assert np.array_equal(R.resize_linear(img, 27, 19), img)                     # identity falls out of the general arithmetic
    for hw, hw2 in GENERAL + [((128, 96), (64, 48)), ((10, 14), (5, 7))]:
        for value in (0, 1, 127, 255):
            out = R.resize_linear(np.full(hw + (3,), value, np.uint8), hw2[1], hw2[0])
            assert out.shape == hw2 + (3,) and (out == value).all(), (hw, hw2, value)


def test_exact_half_size_is_the_rounded_block_mean():
    img = image(10, 14)
    out = R.resize_linear(img, 7, 5)
    v = img.astype(np.int64)
    for y in range(5):
        for x in range(7):
            block = v[2 * y:2 * y + 2, 2 * x:2 * x + 2].reshape(4, 3)
            assert np.array_equal(out[y, x], (block.sum(0) + 2) >> 2), (y, x)
    # half size on one axis only is the general path: the fixed point of two equal weights rounds differently from the block mean
    assert R.is_half_size(10, 14, 5, 7) and not R.is_half_size(10, 14, 5, 8) and not R.is_half_size(10, 14, 6, 7)
    import facelib_oracle as FO
    tall = image(130, 96)
    assert np.array_equal(R.resize_linear(tall, 48, 64), FO.cv2_resize_linear_u8(tall, 48, 64))
    with pytest.raises(NotImplementedError):
        FO.cv2_resize_linear_u8(img, 7, 5)                                       # (the oracle refuses what the restatement adds)


def test_a_row_outside_the_image_keeps_its_weights():
    """Columns outside are moved to the border with weight (2048, 0); rows outside are clamped when read and keep their weights -- on an
    image this is the same value, in the tables it is not, and the kernel's row clamp must not reset b."""
    rows, cols = R.axis_coefficients(3, 8, False), R.axis_coefficients(3, 8, True)
    assert rows[0][0] == -1 and rows[0][1] != 2048 and rows[0][1] + rows[0][2] == 2048      # above the image: s = -1, fractional weights
    assert cols[0] == (0, 2048, 0)                                                           # left of it: reset
    assert rows[-1][0] == 2 and rows[-1][2] != 0                                             # s + 1 = 3 is below the image
    assert cols[-1] == (2, 2048, 0)
    # the two rows a clamped row reads are the same row, so the value is the row's own horizontal pass through both weights
    img = image(3, 5)
    out = R.resize_linear(img, 5, 8)
    hor = img[0].astype(np.int64) * 2048                                                     # identity columns: (x, 2048, 0)
    b0, b1 = rows[0][1], rows[0][2]
    assert np.array_equal(out[0], np.clip((((b0 * (hor >> 4)) >> 16) + ((b1 * (hor >> 4)) >> 16) + 2) >> 2, 0, 255))


def test_header_binding_and_library_agree_on_the_new_symbol():
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    proto = re.search(r'int32_t keep_resize_linear_u8\s*\(([^;]*)\);', header).group(1)
    params = [q.strip() for q in proto.split(',')]
    assert [q.split()[-1].lstrip('*') for q in params] == ['src', 'dst', 'N', 'H', 'W', 'H2', 'W2', 'stream']
    sig = hiplib._CV_SIGNATURES['keep_resize_linear_u8']
    assert sig == [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 5 + [ctypes.c_void_p] and len(sig) == len(params)
    assert 'keep_resize_linear_u8' in hiplib.CV_EXPORTED_SYMBOLS and 'keep_resize_linear_u8' not in hiplib.EXPORTED_SYMBOLS
    assert hiplib.CV_ABI_VERSION == 1 and '#define KEEP_CV_ABI_VERSION 1' in header         # a symbol was added, no prototype changed
    assert hasattr(ctypes.CDLL(hiplib.LIB_PATH), 'keep_resize_linear_u8')
    bound = hiplib.load(check_device=False)
    assert bound.keep_resize_linear_u8.argtypes == sig and bound.keep_resize_linear_u8.restype is ctypes.c_int32


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """Bad arguments never reach a launch: the checks run on the host before anything else, the pointers are never dereferenced."""
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_last_error.restype = ctypes.c_char_p
    f = lib.keep_resize_linear_u8
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 5 + [ctypes.c_void_p]

    def call(src=0x1000, dst=0x1000, N=1, H=90, W=120, H2=64, W2=64):
        return f(src, dst, N, H, W, H2, W2, None)
    for kw in (dict(src=None), dict(dst=None), dict(N=0), dict(N=-1), dict(N=70000), dict(H=0), dict(W=0), dict(H2=0), dict(W2=0),
               dict(H=-5), dict(W2=-1), dict(W=1 << 30), dict(W2=1 << 30), dict(H2=1 << 24)):
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(b'keep_resize_linear_u8'), (kw, lib.keep_last_error())


def test_linear_resizer_argument_checks_need_no_device():
    from comfyui_keep_amd.engine.resize import LinearResizer
    rz = LinearResizer('cpu')
    img = image(9, 11)
    assert rz.resize_u8(img, 11, 9) is img                                       # identity: the input itself, nothing launched
    batch = np.stack([img, img])
    assert rz.resize_u8(batch, 11, 9) is batch
    for bad in (np.zeros((9, 11), np.uint8), np.zeros((9, 11, 4), np.uint8), np.zeros((2, 2, 9, 11, 3), np.uint8)):
        with pytest.raises(ValueError):
            rz.resize_u8(bad, 5, 5)
    with pytest.raises(ValueError):
        rz.resize_u8(np.zeros((9, 11, 3), np.float32), 5, 5)
    with pytest.raises(ValueError):
        rz.resize_u8(img, 5, 5, out=torch.zeros((4, 5, 3), dtype=torch.uint8))


# ---- the processor's choice --------------------------------------------------------------------------------------------------
def _processor(monkeypatch, env):
    from comfyui_keep_amd.modules import keep_processor as KP
    if env is None:
        monkeypatch.delenv('KEEP_AMD_GPU_ALIGNED_RESIZE', raising=False)
    else:
        monkeypatch.setenv('KEEP_AMD_GPU_ALIGNED_RESIZE', env)
    pack = types.SimpleNamespace(keep_net=None, face_helper=types.SimpleNamespace(), bg_upscale_model=None, face_upscale_model=None,
                                 device=torch.device('cpu'), model_type_str='KEEP')
    proc = KP.KEEPFaceProcessor(pack)
    log = {'device': [], 'host': []}

    def device(frames, out=None):
        log['device'].append(tuple(frames.shape))
        return torch.full(tuple(frames.shape[:-3]) + (512, 512, 3), 9, dtype=torch.uint8)

    def host(img, w, h, interp):
        log['host'].append((tuple(img.shape), w, h, interp))
        return np.zeros((h, w) + tuple(img.shape[2:]), img.dtype)
    monkeypatch.setattr(proc, '_aligned_resize_device', device)
    monkeypatch.setattr(KP, '_resize', host)
    return KP, proc, log


def test_knob_forces_the_device_path_on_and_off(monkeypatch):
    img = image(96, 128)
    KP, proc, log = _processor(monkeypatch, '1')
    assert proc.gpu_aligned_resize is True
    out = proc._aligned_face(img)
    assert isinstance(out, np.ndarray) and out.shape == (512, 512, 3) and out.dtype == np.uint8 and (out == 9).all()
    assert log == {'device': [(96, 128, 3)], 'host': []}
    KP, proc, log = _processor(monkeypatch, '0')
    assert proc.gpu_aligned_resize is False
    out = proc._aligned_face(img)
    assert out.shape == (512, 512, 3) and log == {'device': [], 'host': [((96, 128, 3), 512, 512, 'INTER_LINEAR')]}


def test_unset_knob_decides_once_by_cv2(monkeypatch):
    img = image(96, 128)
    # no cv2: the device path is the only resize there is
    KP, proc, log = _processor(monkeypatch, None)
    monkeypatch.setattr(KP, '_cv2', lambda: (_ for _ in ()).throw(ImportError('no cv2')))
    assert proc.gpu_aligned_resize is None
    proc._aligned_face(img)
    assert proc.gpu_aligned_resize is True and len(log['device']) == 1 and not log['host']
    # cv2 imports: the self-check against cv2 decides, once per processor
    for verdict in (True, False):
        KP, proc, log = _processor(monkeypatch, None)
        asked = []
        monkeypatch.setattr(KP, '_cv2', lambda: object())
        monkeypatch.setattr(KP.opencv_checks, 'opencv_agrees_with_gpu_aligned_resize', lambda dev: (asked.append(dev), verdict)[1])
        proc._aligned_face(img)
        proc._aligned_face(img)
        assert asked == [torch.device('cpu')] and proc.gpu_aligned_resize is verdict
        assert (len(log['device']), len(log['host'])) == ((2, 0) if verdict else (0, 2))
    # a self-check that cannot run (no GPU, no library, ...) settles on cv2
    KP, proc, log = _processor(monkeypatch, None)
    monkeypatch.setattr(KP, '_cv2', lambda: object())
    monkeypatch.setattr(KP.opencv_checks, 'opencv_agrees_with_gpu_aligned_resize', lambda dev: (_ for _ in ()).throw(RuntimeError('no device')))
    proc._aligned_face(img)
    assert proc.gpu_aligned_resize is False and not log['device'] and len(log['host']) == 1


def test_a_failing_device_resize_falls_back_and_turns_the_path_off(monkeypatch):
    KP, proc, log = _processor(monkeypatch, '1')
    monkeypatch.setattr(proc, '_aligned_resize_device', lambda *a, **k: (_ for _ in ()).throw(RuntimeError('launch failed')))
    out = proc._aligned_face(image(96, 128))
    assert out.shape == (512, 512, 3) and len(log['host']) == 1 and proc.gpu_aligned_resize is False
    proc._aligned_face(image(96, 128))
    assert len(log['host']) == 2


def test_grey_four_channel_and_16_bit_images_go_to_the_host(monkeypatch):
    KP, proc, log = _processor(monkeypatch, '1')
    for img in (np.zeros((96, 128), np.uint8), np.zeros((96, 128, 4), np.uint8), np.zeros((96, 128, 3), np.uint16),
                np.zeros((96, 128, 3), np.float32), np.zeros((96, 128, 1), np.uint8)):
        log['host'].clear()
        proc._aligned_face(img)
        assert not log['device'] and log['host'] == [(tuple(img.shape), 512, 512, 'INTER_LINEAR')], img.shape
    assert proc.gpu_aligned_resize is True


def test_identity_never_resizes(monkeypatch):
    for env in ('1', '0', None):
        KP, proc, log = _processor(monkeypatch, env)
        monkeypatch.setattr(KP.opencv_checks, 'opencv_agrees_with_gpu_aligned_resize', lambda dev: pytest.fail('self-check at identity'))
        for img in (image(512, 512), np.zeros((512, 512), np.uint8), np.zeros((512, 512, 4), np.uint16)):
            assert proc._aligned_face(img) is img
        assert log == {'device': [], 'host': []} and proc.gpu_aligned_resize is {'1': True, '0': False, None: None}[env]


def test_the_streamed_aligned_form_is_for_one_process_with_device_resizes(monkeypatch):
    """``_aligned_stream_applies``: every condition that keeps the per-frame path, decided without a device."""
    KP, proc, log = _processor(monkeypatch, '1')
    monkeypatch.delenv('KEEP_AMD_STREAM_PASTE', raising=False)
    proc.gpu_resize = True
    proc.keep_net = types.SimpleNamespace(supports_sink=True, pool=None)
    frames = [image(96, 128, seed=i) for i in range(3)]
    assert proc._aligned_stream_applies(frames, 1.0) and proc._aligned_stream_applies(frames, 2.0)
    monkeypatch.setenv('KEEP_AMD_STREAM_PASTE', '0')
    assert not proc._aligned_stream_applies(frames, 1.0)
    monkeypatch.delenv('KEEP_AMD_STREAM_PASTE')
    proc.keep_net = types.SimpleNamespace(supports_sink=False, pool=None)
    assert not proc._aligned_stream_applies(frames, 1.0)
    proc.keep_net = types.SimpleNamespace(supports_sink=True, pool=object())                 # a worker pool: host shares
    assert not proc._aligned_stream_applies(frames, 1.0)
    proc.keep_net = types.SimpleNamespace(supports_sink=True, pool=None)
    proc.face_upscale_model = object()
    assert not proc._aligned_stream_applies(frames, 1.0)
    proc.face_upscale_model = None
    assert not proc._aligned_stream_applies(frames + [image(96, 130)], 1.0)                  # mixed sizes
    assert not proc._aligned_stream_applies([f.astype(np.uint16) for f in frames], 1.0)
    assert not proc._aligned_stream_applies([f[:, :, 0] for f in frames], 1.0)
    proc.gpu_resize = False                                                                   # the output resize is cv2's
    assert proc._aligned_stream_applies(frames, 1.0) and not proc._aligned_stream_applies(frames, 2.0)
    proc.return_restored_aligned = True
    assert proc._aligned_stream_applies(frames, 1.0) and not proc._aligned_stream_applies(frames, 1.5)
    proc.gpu_resize, proc.gpu_aligned_resize = True, False                                    # the input resize is cv2's
    assert not proc._aligned_stream_applies(frames, 1.0)
    assert proc._aligned_stream_applies([image(512, 512, seed=i) for i in range(2)], 1.5)    # ... which 512 x 512 frames do not need
