"""The detector-input resize (cv2.resize INTER_AREA restated: csrc/keep_resize_area.hip, include/keep_cv_hip.h), host side (no GPU): the
library's table builder against the independent numpy restatement (tests/cv_area_ref.py), the refusals of both entry points, the
extension header against the binding and the built library, the frozen core C-ABI, and the processor's choice of who resizes."""
import ctypes
import hashlib
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import cv_area_ref as R
from conftest import ROOT

AXES = ((1080, 640), (1920, 1137), (720, 640), (1280, 1137), (2160, 640), (3840, 1137), (1440, 640), (2560, 1137), (54, 32), (96, 56),
        (45, 40), (80, 71), (48, 16), (64, 21))


def raw_lib():
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_last_error.restype = ctypes.c_char_p
    return lib


def lib_tables(S, D):
    from comfyui_keep_amd.engine.resize import area_tables
    return area_tables(S, D)


@pytest.mark.parametrize('S,D', AXES)
def test_library_tables_equal_the_restatement_entry_for_entry(S, D):
    start, si, alpha = lib_tables(S, D)
    rstart, rsi, ralpha = R.axis_csr(S, D)
    assert start.dtype == np.int32 and si.dtype == np.int32 and alpha.dtype == np.float32
    assert start.shape == (D + 1,) and start[0] == 0 and start[D] == len(si) == len(alpha)
    assert np.array_equal(start, rstart)
    assert np.array_equal(si, rsi)
    assert np.array_equal(alpha.view(np.uint32), ralpha.view(np.uint32)), np.argwhere(alpha.view(np.uint32) != ralpha.view(np.uint32))[:4]


@pytest.mark.parametrize('S,D', AXES)
def test_every_row_has_positive_weights_on_source_pixels_of_the_axis(S, D):
    start, si, alpha = lib_tables(S, D)
    assert (np.diff(start) >= 1).all()                          # a shrinking axis: every destination covers at least one source pixel
    assert (alpha > 0).all() and np.isfinite(alpha).all()
    assert (si >= 0).all() and (si < S).all()
    assert (np.diff(si) >= 0).all()                             # ascending, also across rows: a tile's footprint is [first, last]
    sums = np.add.reduceat(alpha.astype(np.float64), start[:-1])
    # the 1e-3 rule drops a head and a tail of up to 1e-3 source pixels each from a cell of at least one pixel; float32 rounding of at
    # most 10 weights of at most 1 adds less than 1e-6
    assert np.abs(sums - 1).max() <= 2e-3 + 1e-6


def test_table_builder_refusals_name_the_function():
    lib = raw_lib()
    f = lib.keep_area_tables
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 3
    start, si, alpha = (ctypes.c_int32 * 64)(), (ctypes.c_int32 * 256)(), (ctypes.c_float * 256)()
    p = [ctypes.addressof(b) for b in (start, si, alpha)]
    assert f(54, 32, 256, *p) == 0 and start[32] == 84
    for args in ((54, 32, 83, *p),                                # cap one short of the 84 entries
                 (54, 32, 0, *p), (32, 32, 256, *p), (32, 54, 256, *p), (0, 0, 256, *p), (54, -1, 256, *p),
                 (54, 32, 256, None, p[1], p[2]), (54, 32, 256, p[0], None, p[2]), (54, 32, 256, p[0], p[1], None)):
        assert f(*args) == -1, args
        assert lib.keep_last_error().startswith(b'keep_area_tables'), lib.keep_last_error()
    from comfyui_keep_amd.engine import hiplib
    with pytest.raises(hiplib.KeepHipError, match='keep_area_tables'):
        lib_tables(40, 40)


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """Bad arguments never reach a launch: the checks run on the host before anything else (no device is needed to be refused).  The
    pointers are never dereferenced on a refused call."""
    lib = raw_lib()
    f = lib.keep_resize_area_u8
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 5 + [ctypes.c_void_p] * 7
    ptr = [0x1000] * 8                                            # src, dst, xstart, xsi, xalpha, ystart, ysi, yalpha (placeholders)

    def call(N=1, H=1080, W=1920, H2=640, W2=1137, null=None):
        q = list(ptr)
        if null is not None:
            q[null] = None
        return f(q[0], q[1], N, H, W, H2, W2, *q[2:], None)
    refused = [dict(null=i) for i in range(8)]
    refused += [dict(N=0), dict(N=-1), dict(N=70000), dict(H=0), dict(W2=0), dict(H2=-3),
                dict(H2=1080), dict(W2=1920), dict(H2=2160, W2=3840),              # not a shrink on both axes
                dict(H=1280, W=1920, H2=640, W2=960),                              # whole-number scale on both axes: 2 and 2
                dict(H=48, W=64, H2=16, W2=16),                                    # 3 and 4
                dict(H=1080, W=1920, H2=540, W2=960)]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(b'keep_resize_area_u8'), (kw, lib.keep_last_error())
    from comfyui_keep_amd.engine.resize import area_geometry_refused
    assert area_geometry_refused(1280, 1920, 640, 960) and area_geometry_refused(48, 64, 16, 16) and area_geometry_refused(64, 64, 64, 32)
    assert not area_geometry_refused(48, 64, 16, 21) and not area_geometry_refused(1080, 1920, 640, 1137)
    assert R.is_area_fast(1280, 1920, 640, 960) and not R.is_area_fast(48, 64, 16, 21)


def test_extension_header_binding_and_library_agree():
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    declared = set(re.findall(r'\b(keep_[a-z0-9_]+)\s*\(', header))
    assert declared == set(hiplib.CV_EXPORTED_SYMBOLS)
    assert not declared & set(hiplib.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert int(re.search(r'#define KEEP_CV_ABI_VERSION (\d+)', header).group(1)) == hiplib.CV_ABI_VERSION == 1
    lib.keep_cv_abi_version.restype = ctypes.c_int32
    assert lib.keep_cv_abi_version() == 1
    bound = hiplib.load(check_device=False)
    for name, argtypes in hiplib._CV_SIGNATURES.items():
        assert getattr(bound, name).argtypes == argtypes and getattr(bound, name).restype is ctypes.c_int32
    # the prototypes' parameter counts equal the binding's (the stream is the last argument of a launcher)
    for name, argtypes in hiplib._CV_SIGNATURES.items():
        proto = re.search(r'int32_t ' + name + r'\s*\(([^;]*)\);', header).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == len(argtypes), name


def test_core_abi_is_untouched():
    """The area resize came in beside the core C-ABI, not through it: header, version and symbol list are what they were (a change
    of the core ABI itself brings new digests here)."""
    from comfyui_keep_amd.engine import hiplib
    assert hiplib.ABI_VERSION == 23
    header = open(os.path.join(ROOT, 'include', 'keep_hip.h'), 'rb').read()
    assert hashlib.sha256(header).hexdigest() == '47e23f39a554cf5525e978944c4b1b4653adfe976b11d00ae468ee9a161170f0'
    assert b'#define KEEP_ABI_VERSION 23' in header
    assert len(hiplib.EXPORTED_SYMBOLS) == 63 and 'keep_resize_area_u8' not in hiplib.EXPORTED_SYMBOLS
    assert hashlib.sha256('\n'.join(hiplib.EXPORTED_SYMBOLS).encode()).hexdigest() == '26358e1ce07ddc873f4b67a1ad9a6371bde6246840bceb98f7c7d52c5f06ee64'
    syms = subprocess.run(['nm', '-D', '--undefined-only', hiplib.LIB_PATH], capture_output=True, text=True).stdout
    assert 'getenv' not in syms


# ---- the processor's choice --------------------------------------------------------------------------------------------------
class _Helper:
    def clean_all(self):
        pass

    def read_image(self, img):
        self.input_img, self.is_gray = img, False


def _processor(monkeypatch, env, helper=None):
    from comfyui_keep_amd.modules import keep_processor as KP
    if env is None:
        monkeypatch.delenv('KEEP_AMD_GPU_DETECT_RESIZE', raising=False)
    else:
        monkeypatch.setenv('KEEP_AMD_GPU_DETECT_RESIZE', env)
    pack = types.SimpleNamespace(keep_net=None, face_helper=helper or _Helper(), bg_upscale_model=None, face_upscale_model=None,
                                 device=torch.device('cpu'), model_type_str='KEEP')
    proc = KP.KEEPFaceProcessor(pack)
    log = {'device': [], 'host': []}

    def device(imgs, w2, h2):
        log['device'].append((len(imgs), tuple(imgs[0].shape), w2, h2))
        return torch.zeros((len(imgs), h2, w2, 3), dtype=torch.uint8)

    def host(img, w, h, interp):
        log['host'].append((tuple(img.shape), w, h, interp))
        return np.zeros((h, w) + tuple(img.shape[2:]), img.dtype)
    monkeypatch.setattr(proc, '_detect_resize_device', device)
    monkeypatch.setattr(KP, '_resize', host)
    return KP, proc, log


def _frames(n, h=90, w=160, dtype=np.uint8):
    return [np.full((h, w, 3), i, dtype) for i in range(n)]


def test_knob_forces_the_device_path_on_and_off(monkeypatch):
    KP, proc, log = _processor(monkeypatch, '1')
    frames = _frames(3)
    states, batch = proc._prep_detect_chunk(frames, 64)
    assert log == {'device': [(3, (90, 160, 3), 113, 64)], 'host': []}
    assert isinstance(batch, torch.Tensor) and tuple(batch.shape) == (3, 64, 113, 3)
    assert [s[0] is f and s[1] is False for s, f in zip(states, frames)] == [True] * 3
    states, batch = proc._prep_detect_chunk(frames, 64, device_resize=False)          # (the pooled pre-pass: host batches)
    assert len(log['device']) == 1 and log['host'] == [((90, 160, 3), 113, 64, 'INTER_AREA')] * 3 and isinstance(batch, np.ndarray)
    KP, proc, log = _processor(monkeypatch, '0')
    states, batch = proc._prep_detect_chunk(frames, 64)
    assert log == {'device': [], 'host': [((90, 160, 3), 113, 64, 'INTER_AREA')] * 3}
    assert isinstance(batch, np.ndarray) and batch.shape == (3, 64, 113, 3) and len(states) == 3


def test_unset_knob_decides_once_by_cv2(monkeypatch):
    frames = _frames(2)
    # no cv2: the device path is the only resize there is
    KP, proc, log = _processor(monkeypatch, None)
    monkeypatch.setattr(KP, '_cv2', lambda: (_ for _ in ()).throw(ImportError('no cv2')))
    assert proc.gpu_detect_resize is None
    proc._prep_detect_chunk(frames, 64)
    assert proc.gpu_detect_resize is True and len(log['device']) == 1 and not log['host']
    # cv2 imports: the self-check against cv2 decides, once per processor
    for verdict in (True, False):
        KP, proc, log = _processor(monkeypatch, None)
        asked = []
        monkeypatch.setattr(KP, '_cv2', lambda: object())
        monkeypatch.setattr(KP.opencv_checks, 'opencv_agrees_with_gpu_detect_resize', lambda dev: (asked.append(dev), verdict)[1])
        proc._prep_detect_chunk(frames, 64)
        proc._prep_detect_chunk(frames, 64)
        assert asked == [torch.device('cpu')] and proc.gpu_detect_resize is verdict
        assert (len(log['device']), len(log['host'])) == ((2, 0) if verdict else (0, 4))
    # a self-check that cannot run (no GPU, no library, ...) settles on cv2
    KP, proc, log = _processor(monkeypatch, None)
    monkeypatch.setattr(KP, '_cv2', lambda: object())
    monkeypatch.setattr(KP.opencv_checks, 'opencv_agrees_with_gpu_detect_resize', lambda dev: (_ for _ in ()).throw(RuntimeError('no device')))
    proc._prep_detect_chunk(frames, 64)
    assert proc.gpu_detect_resize is False and not log['device'] and len(log['host']) == 2


def test_a_failing_device_resize_falls_back_to_the_present_path(monkeypatch):
    KP, proc, log = _processor(monkeypatch, '1')
    monkeypatch.setattr(proc, '_detect_resize_device', lambda *a: (_ for _ in ()).throw(RuntimeError('launch failed')))
    states, batch = proc._prep_detect_chunk(_frames(2), 64)
    assert len(log['host']) == 2 and isinstance(batch, np.ndarray) and proc.gpu_detect_resize is False


def test_the_helpers_own_resize_wins(monkeypatch):
    class Own(_Helper):
        def __init__(self):
            self.calls = []

        def resize_for_detector(self, img, w, h):
            self.calls.append((w, h))
            return np.zeros((h, w, 3), np.uint8)
    h = Own()
    KP, proc, log = _processor(monkeypatch, '1', h)
    states, batch = proc._prep_detect_chunk(_frames(3), 64)
    assert h.calls == [(113, 64)] * 3 and log == {'device': [], 'host': []} and batch.shape == (3, 64, 113, 3)


def test_mixed_sizes_other_dtypes_and_refused_geometries_take_the_per_frame_path(monkeypatch):
    KP, proc, log = _processor(monkeypatch, '1')
    states, batch = proc._prep_detect_chunk(_frames(2) + _frames(1, 100, 160), 64)      # mixed sizes
    assert not log['device'] and len(log['host']) == 3 and batch is None and len(states) == 3
    log['host'].clear()
    states, batch = proc._prep_detect_chunk(_frames(2, dtype=np.float64), 64)            # what read_image makes of 16-bit sources
    assert not log['device'] and len(log['host']) == 2 and batch is None
    log['host'].clear()
    grey = [np.zeros((90, 160), np.uint8)] * 2                                           # (a helper that leaves a 2-d image)
    proc._prep_detect_chunk(grey, 64)
    assert not log['device'] and len(log['host']) == 2
    log['host'].clear()
    states, batch = proc._prep_detect_chunk(_frames(2, 128, 192), 64)                    # 128x192 -> 64x96: scale 2 on both axes
    assert not log['device'] and log['host'] == [((128, 192, 3), 96, 64, 'INTER_AREA')] * 2 and batch.shape == (2, 64, 96, 3)


def test_frames_within_the_detector_size_launch_nothing(monkeypatch):
    KP, proc, log = _processor(monkeypatch, '1')
    frames = _frames(3, 64, 100)
    states, batch = proc._prep_detect_chunk(frames, 64)                                  # short side == resize: not above it
    assert log == {'device': [], 'host': []} and isinstance(batch, np.ndarray) and np.array_equal(batch, np.stack(frames))
    states, batch = proc._prep_detect_chunk(_frames(2, 40, 50), 64)
    assert log == {'device': [], 'host': []} and batch.shape == (2, 40, 50, 3)
    states, batch = proc._prep_detect_chunk(_frames(2), None)                            # resize=None: the frames as they are
    assert log == {'device': [], 'host': []} and batch.shape == (2, 90, 160, 3)
