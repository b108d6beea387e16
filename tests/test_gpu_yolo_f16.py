"""GPU suite (-m gpu): YOLOv5-face's opt-in single-fp16 precision ('f16': KEEP_MMA_X1 wherever the library's plan admits the call, with
KEEP_CONV_X1_GEMM | KEEP_CONV_X1_HALO16) -- both models against the reference goldens of tests/golden/facelib.npz, the census of planned
kernels, predictions and detections against the x3 engine's, and the untouched default path."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import yoloface as YF

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, 'facelib.npz'))
MODELS = ('YOLOv5n', 'YOLOv5l')
X1_HALO16 = 'conv3x3_halo_x3_kernel<16, 0, false, true, true, false, true>'      # (every YOLO convolution carries SiLU: the general epilogue)
X3_HALO16 = 'conv3x3_halo_x3_kernel<16>'
# The census and the 128 x 128 comparisons plan with this reference batch: the 16 x 16 stride-8 map holds ONE 256-pixel tile, and the form is
# admitted only where KEEP_MMA_X3 plans the call un-split -- 256 reference images x 1 tile x >= 1 cout block = 256 items (what the default 16
# reference images give on the 48 x 80 map of a 720p frame's 768 x 1280 letterbox: 16 x 15 x 4).  A per-engine numerics setting like the precision itself.
REF_IMAGES = 256


def bound_of(measured):
    """1.5 x the measured figure, rounded up to two significant digits."""
    v = 1.5 * measured
    e = int(np.floor(np.log10(v))) - 1
    return float(np.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e)


# max |f16 - reference golden| over the golden prediction tensor (2 x 3 x 96 x 128 inputs): (boxes px, landmarks px, scores), MEASURED on an
# MI355X (2026-10-17); the assertion is 1.5 x the figure rounded up to two significant digits -- the margin covers box-to-box accumulation-order
# differences of split-K partials.  The x3 policy's figures on the same goldens are printed beside them by the test.
GOLD_MEASURED = {'YOLOv5n': (3.1805e-01, 3.2234e-01, 6.0776e-04), 'YOLOv5l': (2.0502e-01, 1.7625e-01, 2.5922e-04)}      # (x3: 3.7e-4 / 4.0e-4 / 5.4e-7 and 1.8e-4 / 2.1e-4 / 2.4e-7; boxes span 561 / 416 px)
# max |f16 - x3| of the 2 x 3 x 128 x 128 predictions (boxes px, landmarks px, scores), same date and rule
X3_MEASURED = {'YOLOv5n': (3.5464e-01, 4.7787e-01, 6.9016e-04), 'YOLOv5l': (1.4566e-01, 2.0129e-01, 2.8014e-04)}
# three 176 x 301 frames through the device path: (largest |conf_f16 - conf_x3| over all prediction rows, largest 1 - IoU between an f16
# detection and its x3 match), same date and rule
DET_MEASURED = {'YOLOv5n': (4.8366e-04, 1.3327e-02), 'YOLOv5l': (1.3953e-04, 3.5253e-01)}      # x3 yields 3321 / 361 detections at conf 0.3
DET_CONF = {'YOLOv5n': 0.3, 'YOLOv5l': 0.3}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def engine(name, precision, ref_images=0):
    eng = YF.YoloFaceEngine(YF.synth_yolo_state_dict(name, seed=0), precision=precision)
    if ref_images:
        eng.o.plan_ref_images = ref_images
    return eng.to('cuda')


def errs(a, b):
    return (float(np.abs(a[..., :4] - b[..., :4]).max()), float(np.abs(a[..., 5:15] - b[..., 5:15]).max()),
            float(np.abs(a[..., [4, 15]] - b[..., [4, 15]]).max()))


def check(tag, got, measured):
    assert measured is not None, f'{tag}: no measured figure recorded yet; this run gives {got}'
    for g, m in zip(got, measured):
        assert g <= bound_of(m), (tag, got, measured)


@pytest.mark.parametrize('name', MODELS)
def test_f16_vs_reference_golden(name):
    x = nhwc(op_input(f'yolo_img_{name}', (2, 3, 96, 128)).mul(0.5).add(0.5).clamp(0, 1))
    ref = G[f'{name.lower()}_pred']
    e16 = errs(engine(name, 'f16').forward_nhwc(x).cpu().numpy(), ref)
    e3 = errs(engine(name, 'x3').forward_nhwc(x).cpu().numpy(), ref)
    print(f'[yolo-f16] {name} golden: f16 box {e16[0]:.4e} px / landmarks {e16[1]:.4e} px / scores {e16[2]:.4e}; x3 {e3[0]:.2e} / {e3[1]:.2e} / {e3[2]:.2e}; '
          f'output scale: boxes {np.abs(ref[..., :4]).max():.0f} px, landmarks {np.abs(ref[..., 5:15]).max():.0f} px, scores 1')
    assert all(a > b for a, b in zip(e16, e3)), 'the f16 engine is as close to the reference as x3: it did not run the single-fp16 kernels'
    check(f'{name} golden', e16, GOLD_MEASURED[name])


def stride8_3x3(name):
    """(Cin, Cout) of every 3x3 stride-1 convolution on the stride-8 map (H / 8): the Bottlenecks of the C3 blocks that run there."""
    out, stride = [], 4
    for i, f, kind, n, c1, c2, args in YF.yolo_layers(name):
        if kind == 'Conv' and args[2] == 2 or kind == 'Shuffle' and args[1] == 2:
            stride *= 2
        elif kind == 'Up':
            stride //= 2
        elif kind == 'C3' and stride == 8:
            out += [(c2 // 2, c2 // 2)] * n
    return out


@pytest.mark.parametrize('name', MODELS)
def test_plan_census(name):
    """One forward at 2 x 3 x 128 x 128 (maps 32 x 32, 16 x 16, 8 x 8, 4 x 4): every 3x3 stride-1 convolution of the stride-8 level with
    Cin % 32 == 0 runs the 16-wide X1 instantiation and none of them x3's 16-wide kernel; the stem and the depthwise layers keep their
    x3 / f32 kernels."""
    x = nhwc(op_input(f'yolo_census_{name}', (2, 3, 128, 128)).mul(0.5).add(0.5).clamp(0, 1))
    census = {}
    for prec in ('x3', 'f16'):
        eng = engine(name, prec, REF_IMAGES)
        eng.o.census = census[prec] = {}
        try:
            eng.forward_nhwc(x)
        finally:
            eng.o.census = None
    want = [c for c in stride8_3x3(name) if c[0] % 32 == 0]
    print(f'[yolo-f16] {name} census x3: {census["x3"]}\n[yolo-f16] {name} census f16: {census["f16"]}')
    assert len(want) >= 1
    assert census['x3'].get(X3_HALO16, 0) == len(want) and X1_HALO16 not in census['x3']
    assert census['f16'].get(X1_HALO16, 0) == len(want) and X3_HALO16 not in census['f16']
    x1 = {k: v for k, v in census['f16'].items() if k not in census['x3']}
    assert sum(x1.values()) > len(want)                                       # the GEMM / im2col / streaming X1 forms run too
    # the Cin = 3 stem (flattened-K exact f32 kernel) is the same launch under both; depthwise layers never come to keep_conv2d
    stem = [k for k in census['x3'] if 'f32' in k or 'c3' in k]
    assert stem and all(census['f16'].get(k) == census['x3'][k] for k in stem), (stem, census)
    assert sum(census['f16'].values()) == sum(census['x3'].values())


@pytest.mark.parametrize('name', MODELS)
def test_f16_vs_x3_predictions(name):
    x = nhwc(op_input(f'yolo_census_{name}', (2, 3, 128, 128)).mul(0.5).add(0.5).clamp(0, 1))
    p16 = engine(name, 'f16', REF_IMAGES).forward_nhwc(x).cpu().numpy()
    p3 = engine(name, 'x3', REF_IMAGES).forward_nhwc(x).cpu().numpy()
    e = errs(p16, p3)
    print(f'[yolo-f16] {name} 128 x 128, f16 against x3: box {e[0]:.4e} px / landmarks {e[1]:.4e} px / scores {e[2]:.4e}')
    assert np.isfinite(p16).all() and e[0] > 0
    check(f'{name} vs x3', e, X3_MEASURED[name])


def kept_rows(eng, frames, conf, cap=4096):
    """The device path of ``yolo_detect_batch_device`` up to the kept rows: per frame [k, 16] (x1 y1 x2 y2 conf ...), network pixels."""
    n, H, W, _ = frames.shape
    (rh, rw), (top, left), (H2, W2) = YF.letterbox_geometry(H, W)
    x = torch.empty((n, H2, W2, 3), device='cuda')
    L.call('keep_yolo_letterbox_u8', torch.from_numpy(frames).cuda(), x, n, H, W, rh, rw, top, left, H2, W2, 1)
    pred = eng.forward_nhwc(x)
    dets = torch.empty((n, cap, 16), device='cuda')
    counts = torch.zeros(n, dtype=torch.int32, device='cuda')
    L.call('keep_yolo_select', pred, dets, counts, n, pred.shape[1], cap, float(conf))
    kept = torch.empty((n, cap, 16), device='cuda')
    kcnt = torch.empty(n, dtype=torch.int32, device='cuda')
    L.call('keep_retina_nms', dets, counts, kept, kcnt, n, cap, 0.5)
    kc = kcnt.cpu().numpy()
    assert (kc >= 0).all(), kc
    return pred.cpu().numpy(), [kept[i, :kc[i]].cpu().numpy() for i in range(n)]


def iou(a, b):
    x1, y1, x2, y2 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1]), np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)


@pytest.mark.parametrize('name', MODELS)
def test_f16_detections_match_x3(name):
    """Three 176 x 301 uint8 frames through letterbox, network, selection and suppression on the device: every f16 detection has an x3
    detection at an IoU distance within the measured bound; an x3 detection whose score lies within the measured score error of the threshold
    (or that was suppressed by / lost to such a neighbour: it has no f16 partner) may be missing -- at most 10 % of x3's detections."""
    frames = np.random.default_rng(11).integers(0, 256, (3, 176, 301, 3), dtype=np.uint8)
    conf = DET_CONF[name]
    p3, k3 = kept_rows(engine(name, 'x3'), frames, conf)
    p16, k16 = kept_rows(engine(name, 'f16'), frames, conf)
    n3 = sum(len(k) for k in k3)
    assert n3 >= 10, f'{name}: x3 alone yields {n3} detections at conf {conf}; lower DET_CONF'
    score_err = float(np.abs(p16[..., 4] * p16[..., 15] - p3[..., 4] * p3[..., 15]).max())
    worst, unmatched16, missing = 0.0, 0, 0
    for a16, a3 in zip(k16, k3):
        used = set()
        for d in a16:
            j = int(np.argmax(iou(d, a3))) if len(a3) else -1
            if j < 0 or iou(d, a3)[j] < 0.5:
                unmatched16 += 1
                continue
            used.add(j)
            worst = max(worst, 1.0 - float(iou(d, a3)[j]))
        missing += len(a3) - len(used)
    print(f'[yolo-f16] {name} detections at conf {conf}: x3 {n3}, f16 {sum(len(k) for k in k16)}; largest 1 - IoU {worst:.4e}, largest score distance {score_err:.4e}; '
          f'f16 detections without an x3 partner {unmatched16}, x3 detections missing under f16 {missing}')
    assert DET_MEASURED[name] is not None, f'{name}: no measured figure recorded yet; this run gives {(score_err, worst)}'
    sb, ib = bound_of(DET_MEASURED[name][0]), bound_of(DET_MEASURED[name][1])
    assert score_err <= sb and worst <= ib
    assert unmatched16 == 0
    excused = 0
    for a16, a3 in zip(k16, k3):
        for j, d in enumerate(a3):
            if not len(a16) or iou(d, a16).max() < 0.5:
                assert abs(float(d[4]) - conf) <= sb, (name, d[:5])
                excused += 1
    assert excused <= 0.1 * n3, (excused, n3)


@pytest.mark.parametrize('name', MODELS)
def test_default_path_is_x3_and_bit_equal(name, monkeypatch):
    import test_detect_precision_host as _stub      # noqa: F401  (the comfy stubs the loader module imports)
    from comfyui_keep_amd.modules import keep_model_loader as KL
    monkeypatch.delenv('KEEP_AMD_DETECT_PRECISION', raising=False)
    sd = YF.synth_yolo_state_dict(name, seed=0)
    h = types.SimpleNamespace(face_parse=None, face_detector=types.SimpleNamespace(detector=types.SimpleNamespace(state_dict=lambda: sd)))
    KL.engine_facelib(h)
    model = h.face_detector.detector
    assert isinstance(model, YF.EngineYoloModel) and model.engine.precision == 'x3' and model.engine.o.blobx1 is None
    x = op_input(f'yolo_img_{name}', (2, 3, 96, 128)).mul(0.5).add(0.5).clamp(0, 1)
    got = model(x.cuda())[0].cpu().numpy()
    assert np.array_equal(got, engine(name, 'x3').forward_nhwc(nhwc(x)).cpu().numpy())
