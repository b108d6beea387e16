"""The batched crop warp (csrc/keep_paste.hip:keep_warp_affine_batch_u8, include/keep_cv_hip.h) and the frame store's plan
(modules/keep_processor.py:frame_store_plan), host side (no GPU): the extension header against the binding and the built library, the
launcher's refusals -- host checks that run before anything is launched --, the rule that cuts F faces into launches, and the decision
whether a sequence's frames stay on the device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAME = 'keep_warp_affine_batch_u8'


def raw_lib():
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_last_error.restype = ctypes.c_char_p
    return lib


def test_symbol_is_in_the_extension_header_the_binding_and_the_library_only():
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    core = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    for name in (NAME, 'keep_warp_batch_group'):
        assert re.search(r'int32_t ' + name + r'\s*\(', header) and name not in core
        assert name in hiplib.CV_EXPORTED_SYMBOLS and name in hiplib._CV_SIGNATURES
        assert name not in hiplib.EXPORTED_SYMBOLS and name not in hiplib._SIGNATURES
        assert hasattr(raw_lib(), name)
        proto = re.search(r'int32_t ' + name + r'\s*\(([^;]*)\);', header).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == len(hiplib._CV_SIGNATURES[name]), name
    assert len(hiplib._CV_SIGNATURES[NAME]) == 14
    assert int(re.search(r'#define KEEP_CV_ABI_VERSION (\d+)', header).group(1)) == hiplib.CV_ABI_VERSION == 1
    bound = hiplib.load(check_device=False)
    assert getattr(bound, NAME).argtypes == hiplib._CV_SIGNATURES[NAME] and getattr(bound, NAME).restype is ctypes.c_int32


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """Every bad argument is refused with KEEP_EINVAL on a machine without a GPU: the checks run on the host before the first launch, and
    the device pointers (placeholders here) are never dereferenced."""
    lib = raw_lib()
    f = getattr(lib, NAME)
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 2 + \
                 [ctypes.c_int32] * 3 + [ctypes.c_void_p]
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]

    def call(N=3, H=37, W=53, F=2, dh=24, dw=40, frame_of=(0, 2), mats=None, null=None):
        idx = (ctypes.c_int32 * max(1, len(frame_of)))(*frame_of)
        m = (ctypes.c_double * (6 * max(1, len(frame_of))))(*(mats if mats is not None else ident * len(frame_of)))
        ptr = [0x1000, 0x2000, ctypes.addressof(idx), ctypes.addressof(m)]             # frames, dst (placeholders), frame_of, dst_to_src
        if null is not None:
            ptr[null] = None
        return f(ptr[0], N, H, W, ptr[1], F, dh, dw, ptr[2], ptr[3], 135, 133, 132, None)
    refused = [dict(null=i) for i in range(4)]
    refused += [dict(N=0), dict(N=-1), dict(F=0), dict(F=-2), dict(H=0), dict(W=0), dict(dh=0), dict(dw=0), dict(H=-5), dict(dw=-1),
                dict(H=32768), dict(W=32768), dict(W=40000),
                dict(frame_of=(0, 3)), dict(frame_of=(-2, 0)), dict(frame_of=(3, 0)), dict(N=1, frame_of=(0, 1)),
                dict(mats=ident + [1.0, 0.0, float('nan'), 0.0, 1.0, 0.0]), dict(mats=[float('inf')] + ident[1:] + ident),
                dict(mats=ident + ident[:5] + [float('-inf')]),
                dict(frame_of=(-1, 0), mats=[float('nan')] + ident[1:] + ident)]      # also the matrix of a black crop must be finite
    for kw in refused:
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(NAME.encode()), (kw, lib.keep_last_error())


@pytest.mark.parametrize('F', [1, 32, 33, 70])
def test_launch_groups_cover_every_face_exactly_once(F):
    """keep_warp_batch_group is the rule the launcher loops over: launch g takes at most 32 faces, the launches of F faces partition
    0 .. F - 1 in order, and there is no launch behind the last."""
    lib = raw_lib()
    f = lib.keep_warp_batch_group
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    first, count = ctypes.c_int32(-7), ctypes.c_int32(-7)
    seen, g = [], 0
    while f(F, g, ctypes.byref(first), ctypes.byref(count)) == 0:
        assert 1 <= count.value <= 32 and first.value == len(seen)
        seen.extend(range(first.value, first.value + count.value))
        g += 1
    assert lib.keep_last_error().startswith(b'keep_warp_batch_group')
    assert seen == list(range(F)) and g == -(-F // 32)
    assert f(F, -1, ctypes.byref(first), ctypes.byref(count)) == -1
    assert f(0, 0, ctypes.byref(first), ctypes.byref(count)) == -1
    assert f(F, 0, None, ctypes.byref(count)) == -1


# ---- the frame store's plan ---------------------------------------------------------------------------------------------------
def _frames(n, h=4, w=6, dtype=np.uint8):
    return [np.zeros((h, w, 3), dtype) for _ in range(n)]


def test_plan_cap_boundary():
    from comfyui_keep_amd.modules.keep_processor import frame_store_plan
    frames = _frames(5)                                            # 5 * 4 * 6 * 3 = 360 bytes
    assert frame_store_plan(frames, 360, 2) == [(0, 2), (2, 4), (4, 5)]     # exactly at the cap: applies
    assert frame_store_plan(frames, 359, 2) is None                         # one byte over: the present path, entirely
    assert frame_store_plan(frames, 10 ** 12, 2) is not None


def test_plan_refuses_mixed_sizes_other_dtypes_and_empty_sequences():
    from comfyui_keep_amd.modules.keep_processor import frame_store_plan
    big = 10 ** 12
    assert frame_store_plan([], big, 4) is None
    assert frame_store_plan(_frames(3) + _frames(1, 5, 6), big, 4) is None
    assert frame_store_plan(_frames(1, 5, 6) + _frames(3), big, 4) is None
    assert frame_store_plan(_frames(3, dtype=np.uint16), big, 4) is None
    assert frame_store_plan(_frames(2) + _frames(1, dtype=np.float32), big, 4) is None
    assert frame_store_plan([np.zeros((4, 6), np.uint8)] * 2, big, 4) is None              # grey
    assert frame_store_plan([np.zeros((4, 6, 4), np.uint8)] * 2, big, 4) is None           # four channels
    assert frame_store_plan(_frames(3), big, 0) is None


@pytest.mark.parametrize('n,chunk', [(1, 32), (32, 32), (33, 32), (10, 4), (7, 1), (96, 32)])
def test_plan_spans_cover_the_sequence_without_overlap(n, chunk):
    from comfyui_keep_amd.modules.keep_processor import frame_store_plan
    spans = frame_store_plan(_frames(n), 10 ** 12, chunk)
    assert spans[0][0] == 0 and spans[-1][1] == n and len(spans) == -(-n // chunk)
    assert all(0 < b - a <= chunk for a, b in spans) and all(b - a == chunk for a, b in spans[:-1])
    assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))
    assert [t for a, b in spans for t in range(a, b)] == list(range(n))


def test_knob_and_failure_turn_the_store_off_without_a_device(monkeypatch):
    """KEEP_AMD_FRAME_STORE=0 and a processor whose store failed once answer None before anything else is asked."""
    import types
    import torch
    from comfyui_keep_amd.modules import keep_processor as KP
    pack = types.SimpleNamespace(keep_net=None, face_helper=types.SimpleNamespace(), bg_upscale_model=None, face_upscale_model=None,
                                 device=torch.device('cpu'), model_type_str='KEEP')
    proc = KP.KEEPFaceProcessor(pack)
    assert proc.frame_store is True
    monkeypatch.setenv('KEEP_AMD_FRAME_STORE', '0')
    assert proc._frame_store_begin(_frames(3)) is None
    monkeypatch.delenv('KEEP_AMD_FRAME_STORE')
    assert proc._frame_store_begin(_frames(3)) is None             # (no detector that takes batches, no engine net)
    store = KP._FrameStore([(0, 2), (2, 3)], 4, 6, torch.device('cpu'))
    proc._frame_store_failed(store, RuntimeError('launch failed'))
    assert proc.frame_store is False and store.dead and store.bufs == [None, None]
