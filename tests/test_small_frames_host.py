"""Small frames -- ``read_image``'s enlargement of a frame whose short side is below 512 (face_restoration_helper.py:182-184) on the device:
csrc/keep_resize_linear.hip:keep_resize_linear_fxy_u8, engine/resize.py:LinearResizer.enlarge_u8, the small-frame form of the frame
store in modules/keep_processor.py -- host side (no GPU): the extension header against the binding and the built library, the
launcher's refusals, the independent restatement (tests/cv_linear_fxy_ref.py) pinned to the pinned one and shown to discriminate, and the
processor's routing over recording fakes."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import cv_linear_fxy_ref as F
import cv_linear_ref as R
from conftest import ROOT

NAME = 'keep_resize_linear_fxy_u8'


def image(h, w, seed=None):
    return np.random.default_rng(h * 1000 + w if seed is None else seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- symbol ---------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_symbol():
    from comfyui_keep_amd.engine import hiplib
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    core = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    proto = re.search(r'int32_t ' + NAME + r'\s*\(([^;]*)\);', header).group(1)
    params = [q.strip() for q in proto.split(',')]
    assert [q.split()[-1].lstrip('*') for q in params] == ['src', 'dst', 'N', 'H', 'W', 'H2', 'W2', 'fx', 'fy', 'stream']
    assert [q.split()[0] for q in params[7:9]] == ['double', 'double']
    sig = hiplib._CV_SIGNATURES[NAME]
    assert sig == [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 5 + [ctypes.c_double] * 2 + [ctypes.c_void_p]
    assert NAME in hiplib.CV_EXPORTED_SYMBOLS and NAME not in hiplib.EXPORTED_SYMBOLS and NAME not in core
    assert hiplib.CV_ABI_VERSION == 1 and '#define KEEP_CV_ABI_VERSION 1' in header         # a symbol was added, no prototype changed
    raw = ctypes.CDLL(hiplib.LIB_PATH)
    assert hasattr(raw, NAME)
    raw.keep_cv_abi_version.restype = ctypes.c_int32
    assert raw.keep_cv_abi_version() == 1
    bound = hiplib.load(check_device=False)
    assert getattr(bound, NAME).argtypes == sig and getattr(bound, NAME).restype is ctypes.c_int32
    # the dsize entry's prototype is what it was
    old = re.search(r'int32_t keep_resize_linear_u8\s*\(([^;]*)\);', header).group(1)
    assert [q.split()[-1].lstrip('*') for q in old.split(',')] == ['src', 'dst', 'N', 'H', 'W', 'H2', 'W2', 'stream']


def test_launcher_refusals_are_host_checks_that_name_the_function():
    """Bad arguments never reach a launch: the checks run on the host before anything else, the pointers are never dereferenced."""
    from comfyui_keep_amd.engine import hiplib
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    lib.keep_last_error.restype = ctypes.c_char_p
    f = getattr(lib, NAME)
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int32] * 5 + [ctypes.c_double] * 2 + [ctypes.c_void_p]
    fac = 512.0 / 360

    def call(src=0x1000, dst=0x1000, N=1, H=360, W=480, H2=512, W2=683, fx=fac, fy=fac):
        return f(src, dst, N, H, W, H2, W2, fx, fy, None)
    bad = [dict(src=None), dict(dst=None), dict(N=0), dict(N=-1), dict(N=70000), dict(H=0), dict(W=-3), dict(H2=0), dict(W2=-1),
           dict(fx=0.0), dict(fy=-1.0), dict(fx=math.inf), dict(fy=math.nan), dict(fx=math.nan),
           dict(W2=682), dict(W2=684), dict(H2=511), dict(H2=513),
           dict(fx=1.0 / (683.0 / 480.0)), dict(W2=640, H2=480),                       # (sizes that fit the dsize form, not these factors)
           dict(H=1, W=1, H2=1, W2=1, fx=1e-3, fy=1e-3),                               # the rounded product is 0
           dict(W=1 << 20, W2=1 << 30, fx=1024.0, H=1, H2=1, fy=1.0)]                  # W2 * 3 overflows int32
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.keep_last_error().startswith(NAME.encode()), (kw, lib.keep_last_error())
    # ties go to even: 5 * 0.5 = 2.5 -> 2, 7 * 0.25 = 1.75 -> 2, 6 * 0.25 = 1.5 -> 2
    assert call(H=5, W=7, H2=3, W2=2, fx=0.25, fy=0.5) == -1 and call(H=5, W=6, H2=2, W2=1, fx=0.25, fy=0.5) == -1
    # the exact 2x shrink is cv2's INTER_AREA path: refused, not restated
    assert call(H=10, W=14, H2=5, W2=7, fx=0.5, fy=0.5) == -1 and b'INTER_AREA' in lib.keep_last_error()


def test_linear_resizer_enlarge_argument_checks_need_no_device():
    from comfyui_keep_amd.engine.resize import LinearResizer
    rz = LinearResizer('cpu')
    assert LinearResizer.enlarged_size(360, 480, 512.0 / 360, 512.0 / 360) == (683, 512)
    assert LinearResizer.enlarged_size(480, 270, 512.0 / 270, 512.0 / 270) == (512, 910)
    assert LinearResizer.enlarged_size(5, 7, 0.5, 0.5) == (4, 2)                             # ties to even
    for h, w in ((360, 480), (480, 270), (240, 320), (240, 426), (511, 600), (1, 7), (300, 400), (480, 854)):
        f = 512.0 / min(h, w)
        assert LinearResizer.enlarged_size(h, w, f, f) == F.enlarged_size(h, w, f, f)
    img = image(9, 11)
    for bad in (np.zeros((9, 11), np.uint8), np.zeros((9, 11, 4), np.uint8), np.zeros((2, 2, 9, 11, 3), np.uint8)):
        with pytest.raises(ValueError):
            rz.enlarge_u8(bad, 2.0, 2.0)
    with pytest.raises(ValueError):
        rz.enlarge_u8(np.zeros((9, 11, 3), np.float32), 2.0, 2.0)
    for fx, fy in ((0.0, 2.0), (2.0, -1.0), (math.nan, 2.0), (2.0, math.inf), (1e-3, 2.0)):
        with pytest.raises(ValueError):
            rz.enlarge_u8(img, fx, fy)
    with pytest.raises(ValueError):
        rz.enlarge_u8(img, 2.0, 2.0, out=torch.zeros((18, 21, 3), dtype=torch.uint8))


# ---- restatement ----------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_pinned_one_where_the_two_scales_coincide():
    img = image(37, 53, seed=3)
    assert F.enlarged_size(37, 53, 2.0, 2.0) == (106, 74)
    assert np.array_equal(F.resize_linear_fxy(img, 2.0, 2.0), R.resize_linear(img, 106, 74))


@pytest.mark.parametrize('hw,hw2', [((360, 480), (512, 683)), ((480, 270), (910, 512))])
def test_the_product_geometries_discriminate_between_the_two_forms(hw, hw2):
    """1 / f is not 1 / (D / S) once the size has been rounded: the two forms give different pixels."""
    h, w = hw
    f = 512.0 / min(h, w)
    assert F.enlarged_size(h, w, f, f) == (hw2[1], hw2[0])
    assert 1.0 / f != 1.0 / (float(max(hw2)) / max(hw))
    img = image(h, w)
    got = F.resize_linear_fxy(img, f, f)
    assert got.shape == hw2 + (3,) and got.dtype == np.uint8
    assert (got != R.resize_linear(img, hw2[1], hw2[0])).any()
    for value in (0, 255):
        assert (F.resize_linear_fxy(np.full((h, w, 3), value, np.uint8), f, f) == value).all()


# ---- routing --------------------------------------------------------------------------------------------------------------------
class _Helper:
    """Records its ``read_image`` calls; ``enlarges`` makes it behave like face_restoration_helper.py:182-184."""
    use_parse, pad_blur = True, False
    face_size = (512, 512)
    det_model = 'retinaface_resnet50'

    def __init__(self, enlarges):
        self.enlarges, self.reads = enlarges, 0
        self.face_template = np.zeros((5, 2))
        self.face_parse = types.SimpleNamespace(engine=object())
        self.face_detector = types.SimpleNamespace(detect_batch=None, engine=types.SimpleNamespace(max_frames=4))

    def clean_all(self):
        pass

    def read_image(self, img):
        self.reads += 1
        self.input_img, self.is_gray = img, False
        if self.enlarges and min(img.shape[:2]) < 512:
            f = 512.0 / min(img.shape[:2])
            self.input_img = F.resize_linear_fxy(img, f, f)

    def estimate_similarity(self, lm):
        return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


class _Store:
    """A recording stand-in for ``_FrameStore``: what the processor asks of it, without a device."""

    def __init__(self, spans, cap_bytes=None):
        self.spans, self.cap_bytes, self.small, self.dead = spans, cap_bytes, None, False
        self.filled, self.enlarged, self.dropped = {}, {}, 0
        self.bufs, self.ebufs = [None] * len(spans), [None] * len(spans)

    def fill(self, k, frames):
        self.filled[k] = list(frames)
        self.bufs[k] = torch.zeros((len(frames),) + tuple(frames[0].shape), dtype=torch.uint8)
        return self.bufs[k]

    def enlarge(self, k, resizer):
        f, h2, w2 = self.small
        self.enlarged[k] = f
        self.ebufs[k] = torch.zeros((self.bufs[k].shape[0], h2, w2, 3), dtype=torch.uint8)
        return self.ebufs[k]

    def drop(self, stream=None):
        self.dropped += 1


def _processor(monkeypatch, helper, env='1', **pack):
    from comfyui_keep_amd.modules import keep_processor as KP
    for name, value in (('KEEP_AMD_GPU_SMALL_FRAMES', env), ('KEEP_AMD_FRAME_STORE', None), ('KEEP_AMD_FRAME_STORE_GB', None),
                        ('KEEP_AMD_STREAM_PASTE', None)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    net = types.SimpleNamespace(supports_sink=True, pool=None)
    kw = dict(keep_net=net, face_helper=helper, bg_upscale_model=None, face_upscale_model=None, device=torch.device('cuda', 0),
              model_type_str='KEEP')
    kw.update(pack)
    proc = KP.KEEPFaceProcessor(types.SimpleNamespace(**kw))
    proc.gpu_paste = proc.gpu_resize = True
    return KP, proc


def _video(n=6, h=360, w=480):
    return [image(h, w, seed=i) for i in range(n)]


def _prep_all(proc, store, frames, chunk=4):
    return [proc._prep_detect_chunk(frames[a:b], 640, store=store, k=k) for k, (a, b) in enumerate(store.spans)]


def test_a_helper_that_enlarges_takes_the_new_path_with_one_read_image(monkeypatch):
    helper = _Helper(enlarges=True)
    KP, proc = _processor(monkeypatch, helper)
    frames = _video()
    frames[2] = np.repeat(frames[2][:, :, :1], 3, axis=2)                                   # a grey frame among them
    store = proc._frame_store_begin(frames)
    assert isinstance(store, KP._FrameStore) and store.spans == [(0, 4), (4, 6)] and store.small is None and store.cap_bytes == 16e9
    store = _Store(store.spans, store.cap_bytes)
    out = _prep_all(proc, store, frames)
    assert helper.reads == 1                                                                # the probe, and nothing after it
    assert store.small == (512.0 / 360, 512, 683) and not store.dead
    # the store holds both chunks, twice: the original frames and their enlargement
    assert sorted(store.filled) == sorted(store.enlarged) == [0, 1]
    assert all(a is b for a, b in zip(store.filled[0] + store.filled[1], frames))
    for (states, batch), k in zip(out, (0, 1)):
        assert batch is store.ebufs[k] and tuple(batch.shape) == (len(store.filled[k]), 512, 683, 3)      # the detector batch itself
        assert [tuple(s[0].shape) for s in states] == [(512, 683, 3)] * len(states)
    assert [s[1] for states, _ in out for s in states] == [False, False, True, False, False, False]      # _is_gray(frame)


def test_an_identity_helper_takes_exactly_todays_calls(monkeypatch):
    helper = _Helper(enlarges=False)
    KP, proc = _processor(monkeypatch, helper)
    frames = _video()
    store = _Store([(0, 4), (4, 6)], 16e9)
    out = _prep_all(proc, store, frames)
    assert helper.reads == 6 and store.small is None and not store.dead and not store.enlarged
    assert all(a is b for a, b in zip(store.filled[0] + store.filled[1], frames))
    for (states, batch), k in zip(out, (0, 1)):
        assert batch is store.bufs[k]                                                       # no detector resize: the stored chunk
        assert all(s[0] is f and s[1] is False for s, f in zip(states, store.filled[k]))


def test_knob_off_cap_and_host_lanczos_keep_the_present_handling(monkeypatch):
    frames = _video()
    for case in ('knob', 'cap', 'lanczos'):
        helper = _Helper(enlarges=True)
        KP, proc = _processor(monkeypatch, helper, env='0' if case == 'knob' else '1')
        assert proc.gpu_small_frames is (case != 'knob')
        if case == 'lanczos':
            proc.gpu_resize = False                                                         # the backgrounds could not be resized on the device
        # both copies count against the cap: 6 * (360 * 480 + 512 * 683) * 3 bytes
        store = _Store([(0, 4), (4, 6)], 6 * (360 * 480 + 512 * 683) * 3 - (1 if case == 'cap' else 0))
        out = _prep_all(proc, store, frames)
        assert helper.reads == 6 and store.dead and store.small is None and not store.filled and not store.enlarged, case
        assert all(isinstance(b, np.ndarray) and b.shape[1:] == (512, 683, 3) for _, b in out)            # the helper's own frames
    helper = _Helper(enlarges=True)
    KP, proc = _processor(monkeypatch, helper)
    store = _Store([(0, 4), (4, 6)], 6 * (360 * 480 + 512 * 683) * 3)                       # exactly the cap still applies
    _prep_all(proc, store, frames)
    assert helper.reads == 1 and store.small is not None and not store.dead


def test_a_read_image_that_changes_frames_otherwise_ends_the_store_as_before(monkeypatch):
    class Other(_Helper):
        def read_image(self, img):
            super().read_image(img)
            self.input_img = np.ascontiguousarray(self.input_img[:-1])                      # not the reference's enlargement
    helper = Other(enlarges=True)
    KP, proc = _processor(monkeypatch, helper)
    store = _Store([(0, 4), (4, 6)], 16e9)
    _prep_all(proc, store, _video())
    assert helper.reads == 6 and store.dead and store.small is None and not store.filled
    # frames of 512 and above are not enlarged: today's store
    helper = _Helper(enlarges=True)
    KP, proc = _processor(monkeypatch, helper)
    store = _Store([(0, 2)], 16e9)
    _prep_all(proc, store, _video(2, 512, 600))
    assert helper.reads == 2 and store.small is None and not store.dead and sorted(store.filled) == [0]


def test_grey_16_bit_four_channel_mixed_sources_a_pool_and_an_upscale_model_have_no_store(monkeypatch):
    helper = _Helper(enlarges=True)
    KP, proc = _processor(monkeypatch, helper)
    frames = _video()
    assert proc._frame_store_begin(frames) is not None
    assert proc._frame_store_begin([f[:, :, 0] for f in frames]) is None                    # grey
    assert proc._frame_store_begin([f.astype(np.uint16) * 257 for f in frames]) is None     # 16-bit
    assert proc._frame_store_begin([np.dstack([f, f[:, :, :1]]) for f in frames]) is None   # 4 channels
    assert proc._frame_store_begin(frames[:3] + _video(1, 368, 480)) is None                # mixed sizes
    assert helper.reads == 0                                                                # (decided before the probe)
    KP, proc = _processor(monkeypatch, helper)
    proc.keep_net.pool = object()
    assert proc._frame_store_begin(frames) is None
    KP, proc = _processor(monkeypatch, helper, bg_upscale_model=object())
    assert proc._frame_store_begin(frames) is None
    KP, proc = _processor(monkeypatch, helper)
    monkeypatch.setenv('KEEP_AMD_FRAME_STORE', '0')
    assert proc._frame_store_begin(frames) is None


def test_a_frame_without_a_face_drops_the_small_frame_store_before_anything_is_warped(monkeypatch):
    from comfyui_keep_amd.engine import paste
    helper = _Helper(enlarges=True)
    KP, proc = _processor(monkeypatch, helper)
    monkeypatch.setattr(paste, 'crop_faces_batch', lambda *a, **k: pytest.fail('warped'))
    monkeypatch.setattr(proc, '_restore_and_paste_streamed', lambda *a, **k: pytest.fail('restored'))
    frames = _video()
    track = np.zeros((6, 5, 2))
    track[3] = np.nan
    store = _Store([(0, 4), (4, 6)], 16e9)
    store.small = (512.0 / 360, 512, 683)
    assert proc._stored_sequence(store, frames, {0: track}, 4, 1.0, False, None, True) is None
    assert store.dropped == 1 and proc.frame_store is True                                  # no failure: the present path, quietly


def test_unset_knob_decides_once_by_cv2(monkeypatch):
    frame, big = image(360, 480), np.zeros((512, 683, 3), np.uint8)
    KP, proc = _processor(monkeypatch, _Helper(True), env=None)
    monkeypatch.setattr(KP, '_cv2', lambda: (_ for _ in ()).throw(ImportError('no cv2')))
    assert proc.gpu_small_frames is None
    assert proc._small_frames_probe(_Store([(0, 1)]), 1, frame, big) and proc.gpu_small_frames is True
    for verdict in (True, False):
        KP, proc = _processor(monkeypatch, _Helper(True), env=None)
        asked = []
        monkeypatch.setattr(KP, '_cv2', lambda: object())
        monkeypatch.setattr(KP.opencv_checks, 'opencv_agrees_with_gpu_small_frame_resize', lambda dev: (asked.append(dev), verdict)[1])
        assert proc._small_frames_probe(_Store([(0, 1)]), 1, frame, big) is verdict
        assert proc._small_frames_probe(_Store([(0, 1)]), 1, frame, big) is verdict
        assert asked == [torch.device('cuda', 0)] and proc.gpu_small_frames is verdict
    KP, proc = _processor(monkeypatch, _Helper(True), env=None)
    monkeypatch.setattr(KP, '_cv2', lambda: object())
    monkeypatch.setattr(KP.opencv_checks, 'opencv_agrees_with_gpu_small_frame_resize', lambda dev: (_ for _ in ()).throw(RuntimeError('no device')))
    assert not proc._small_frames_probe(_Store([(0, 1)]), 1, frame, big) and proc.gpu_small_frames is False
    # a frame the probe does not take never runs the self-check
    KP, proc = _processor(monkeypatch, _Helper(True), env=None)
    monkeypatch.setattr(KP.opencv_checks, 'opencv_agrees_with_gpu_small_frame_resize', lambda dev: pytest.fail('self-check'))
    assert not proc._small_frames_probe(_Store([(0, 1)]), 1, image(600, 800), image(600, 800))
    assert not proc._small_frames_probe(_Store([(0, 1)]), 1, frame, big[:-1])
    assert not proc._small_frames_probe(_Store([(0, 1)]), 1, frame, big.astype(np.float64))
    assert proc.gpu_small_frames is None


def test_the_per_frame_paste_resizes_the_background_only_for_read_images_enlargement(monkeypatch):
    helper = _Helper(enlarges=True)
    KP, proc = _processor(monkeypatch, helper)
    log = []
    monkeypatch.setattr(proc, '_lanczos', lambda img, w, h, on_device=False: (log.append(('lanczos', tuple(img.shape), w, h, on_device)),
                                                                               np.zeros((h, w, 3), np.uint8))[1])
    monkeypatch.setattr(proc, '_paste_gpu', lambda h, bg, draw_box=False: (log.append(('gpu', tuple(bg.shape))), 'gpu')[1])
    helper.paste_faces_to_input_image = lambda upsample_img=None, **kw: (log.append(('helper', tuple(upsample_img.shape))), 'helper')[1]
    helper.restored_faces = [np.zeros((512, 512, 3), np.uint8)]
    helper.inverse_affine_matrices = [np.eye(2, 3)]
    helper.input_img = np.zeros((512, 683, 3), np.uint8)
    helper.upscale_factor = 2.0
    bg = np.zeros((600, 800, 3), np.uint8)                                                  # 300 x 400 times 2
    assert proc._paste(helper, bg, False, src_hw=(300, 400)) == 'gpu'
    assert log == [('lanczos', (600, 800, 3), 1366, 1024, True), ('gpu', (1024, 1366, 3))]
    log.clear()
    assert proc._paste(helper, bg, False) == 'helper' and log == [('helper', (600, 800, 3))]          # no source size: as before
    log.clear()
    assert proc._paste(helper, bg, False, src_hw=(368, 480)) == 'helper'                    # the helper holds another frame: as before
    proc.gpu_small_frames = False
    assert proc._paste(helper, bg, False, src_hw=(300, 400)) == 'helper'
    proc.gpu_small_frames, proc.gpu_resize = True, False
    assert proc._paste(helper, bg, False, src_hw=(300, 400)) == 'helper'
    proc.gpu_resize = True
    helper.restored_faces = [np.zeros((256, 256, 3), np.uint8)]                             # something else fails too
    assert proc._paste(helper, bg, False, src_hw=(300, 400)) == 'helper'
    assert [e[0] for e in log] == ['helper'] * 4
    # a background of the right size is pasted as before, untouched
    log.clear()
    helper.restored_faces = [np.zeros((512, 512, 3), np.uint8)]
    assert proc._paste(helper, np.zeros((1024, 1366, 3), np.uint8), False, src_hw=(300, 400)) == 'gpu' and log == [('gpu', (1024, 1366, 3))]
