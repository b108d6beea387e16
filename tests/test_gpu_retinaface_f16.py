"""GPU suite (-m gpu): RetinaFace's opt-in single-fp16 precision ('f16': KEEP_MMA_X1 wherever the library's plan admits the call, with
KEEP_CONV_X1_GEMM) -- both backbones against the reference goldens of tests/golden/facelib.npz, the census of planned kernels, the
detections against the x3 engine's, batch invariance and the untouched default path."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import retinaface as RF

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, 'facelib.npz'))


def bound_of(measured):
    """1.25 x the measured figure, rounded up to two significant digits."""
    v = 1.25 * measured
    e = int(np.floor(np.log10(v))) - 1
    return float(np.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e)


# max |f16 - reference golden| per key over the golden head outputs (2 x 3 x 160 x 224 inputs), MEASURED on an MI355X (2026-10-17); the
# assertion is 1.25 x the figure rounded up to two significant digits (the kernels are deterministic; the margin covers another plan
# choice).  The x3 policy's figure on the same goldens is printed beside it by the test.
E16_MEASURED = {'retinaface_loc': 2.2513e-02, 'retinaface_conf': 4.7319e-03, 'retinaface_landm': 2.5396e-02,      # (x3: 2.5e-5 / 5.6e-6 / 2.9e-5)
                'mnet_loc': 1.4952e-02, 'mnet_conf': 3.7815e-03, 'mnet_landm': 1.4565e-02}                            # (x3: 1.1e-5 / 2.7e-6 / 1.3e-5)
E16_BOUND = {k: bound_of(v) for k, v in E16_MEASURED.items()}      # 0.029 / 0.0060 / 0.032 and 0.019 / 0.0048 / 0.019
# detections of the 3 x 150 x 210 uint8 frames (resnet50: seed 3, threshold 0.8; mobile0.25: seed 5, threshold 0.7) against the x3 engine's:
# the largest |score_f16 - score_x3| over all anchors, and the largest box / landmark distance in pixels between matched detections
DET_MEASURED = {'resnet50': (7.3273e-03, 2.4879), 'mobile0.25': (5.1583e-03, 3.4763e-01)}      # (score error, pixels); 155 / 236 x3 detections
DET_BOUND = {k: tuple(bound_of(x) for x in v) for k, v in DET_MEASURED.items()}                  # (0.0092, 3.2) and (0.0065, 0.44)
DETECT = {'resnet50': (3, 0.8), 'mobile0.25': (5, 0.7)}
GOLD = {'resnet50': ('retinaface_img', 'retinaface_loc', 'retinaface_conf', 'retinaface_landm'),
        'mobile0.25': ('retinaface_mnet_img', 'mnet_loc', 'mnet_conf', 'mnet_landm')}

X1_GEMM = ('conv_x3_kernel<2, 2, 1, 1, true, 1, 0, 1, 0, 1>', 'conv_x3_kernel<2, 2, 2, 2, true, 1, 0, 1, 0, 1>')
X1_IM2COL = ('conv_x3_kernel<2, 2, 1, 1, true, 0, 0, 1, 0, 1>', 'conv_x3_kernel<2, 2, 2, 2, true, 0, 0, 1, 0, 1>')
X1_HALO = 'conv3x3_halo_x3s_kernel<0, false, true>'


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def engine(backbone, precision):
    W = RF.synth_retinaface_state_dict(seed=0, backbone=backbone)
    return RF.RetinaFaceEngine(W, precision=precision).to('cuda')


def heads(eng, x):
    loc, cls, lm = (t.cpu() for t in eng.raw_outputs(x))
    return loc.numpy(), torch.softmax(cls, -1).numpy(), lm.numpy()


@pytest.mark.parametrize('backbone', ['resnet50', 'mobile0.25'])
def test_f16_against_the_reference_goldens(backbone):
    img, *keys = GOLD[backbone]
    x = nhwc(op_input(img, (2, 3, 160, 224), 100.0))
    eng = engine(backbone, 'f16')
    assert eng.o.mma == L.MMA_X3 and eng.o.blobx1 is not None and eng.o.x1_flags == L.CONV_X1_GEMM and eng.o.x1_base_kernel is None
    got16, got3 = heads(eng, x), heads(engine(backbone, 'x3'), x)
    errs = {}
    for g16, g3, key in zip(got16, got3, keys):
        errs[key] = float(np.abs(g16 - G[key]).max())
        e3 = float(np.abs(g3 - G[key]).max())
        print(f'[f16-retinaface] {backbone} {key}: E16 {errs[key]:.4e} (x3 against the same golden {e3:.3e}; scale {np.abs(G[key]).max():.2f})')
        assert np.isfinite(g16).all()
        assert errs[key] > 4 * e3, key                       # really the single-fp16 kernels
    for key in keys:
        assert errs[key] <= E16_BOUND[key], (key, errs[key])


def test_plan_census_resnet50():
    """One resnet50 forward at 2 x 160 x 224: every 1x1 stride-1 convolution with whole 32-channel K steps is planned onto the x1 GEMM
    instantiation, the Cin = 3 stem onto an exact-f32 kernel, and -- no map of this size is tileable -- every other convolution onto the x1
    im2col form."""
    eng = engine('resnet50', 'f16')
    x = nhwc(op_input('retinaface_img', (2, 3, 160, 224), 100.0))
    eng.o.profile = []
    try:
        eng.raw_heads(x)
        torch.cuda.synchronize()
        launches = [(p[0], p[6]) for p in eng.o.profile]
    finally:
        eng.o.profile = None
    n_gemm = n_stem = n_other = 0
    for kernel, (N, H, W, Cin, Cout, KH, stride, up, pro) in launches:
        if Cin == 3:
            assert KH == 7 and kernel.startswith('conv_f32_kernel'), (kernel, Cin, KH)
            n_stem += 1
        elif KH == 1 and stride == 1:
            assert Cin % 32 == 0 and kernel in X1_GEMM, (kernel, H, W, Cin, Cout)
            n_gemm += 1
        else:
            assert kernel in X1_IM2COL, (kernel, H, W, Cin, Cout, KH, stride)
            n_other += 1
    # 16 Bottlenecks x 2 + the stride-1 downsample of layer1 + 3 FPN laterals + 3 fused heads; 3 stride-2 downsamples are im2col shapes
    assert (n_stem, n_gemm) == (1, 16 * 2 + 1 + 3 + 3), (n_stem, n_gemm, n_other)
    assert n_other == 3 + 16 + 2 + 15
    print(f'[f16-retinaface] census: {n_gemm} x1 GEMM launches, {n_other} x1 im2col launches, {n_stem} f32 stem')


def _decoded(eng, frames, cfg, H, W):
    x = frames.float().cuda() - torch.tensor(RF.MEAN_BGR, device='cuda')
    loc, conf, lm = heads(eng, x.contiguous())
    pri = RF.prior_boxes(H, W, cfg)
    boxes = [RF.decode_boxes(loc[i], pri, cfg['variance']) * np.array([W, H, W, H], np.float32) for i in range(len(frames))]
    return conf[..., 1], boxes


@pytest.mark.parametrize('backbone', ['resnet50', 'mobile0.25'])
def test_detections_against_x3(backbone):
    seed, thr = DETECT[backbone]
    frames = torch.randint(0, 256, (3, 150, 210, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    e16, e3 = engine(backbone, 'f16'), engine(backbone, 'x3')
    d16, d3 = e16.detect_batch(frames, conf_threshold=thr), e3.detect_batch(frames, conf_threshold=thr)
    for i in range(3):                                       # a frame's detections never depend on its batch-mates
        one = e16.detect_batch(frames[i:i + 1], conf_threshold=thr)[0]
        assert one.dtype == d16[i].dtype and np.array_equal(one.view(np.int32), d16[i].view(np.int32)), i
    sc16, box16 = _decoded(e16, frames, e16.cfg, 150, 210)
    sc3, _ = _decoded(e3, frames, e3.cfg, 150, 210)
    score_err = float(np.abs(sc16 - sc3).max())
    n3 = sum(len(d) for d in d3)
    near = sum(int((np.abs(d[:, 4] - thr) <= score_err).sum()) for d in d3)
    dist, matched, skipped = 0.0, 0, 0
    for i in range(3):
        for d in d16[i]:
            j = int(np.argmin(np.abs(box16[i] - d[:4]).sum(1)))                      # the anchor of this f16 detection
            assert np.abs(box16[i][j] - d[:4]).max() <= 1e-2
            if abs(sc3[i, j] - thr) <= score_err:
                skipped += 1
                continue
            assert len(d3[i]), (i, d[:5])
            k = int(np.argmin(np.abs(d3[i][:, :4] - d[:4]).sum(1)))
            dist = max(dist, float(np.abs(d3[i][k, :4] - d[:4]).max()), float(np.abs(d3[i][k, 5:] - d[5:]).max()))
            matched += 1
    n16 = sum(len(d) for d in d16)
    print(f'[f16-retinaface] {backbone} detections at {thr}: x3 {n3}, f16 {n16} ({matched} matched, {skipped} with an x3 score within the score '
          f'error of the threshold); score error {score_err:.4e}; largest box / landmark distance {dist:.4e} px; '
          f'{near} of {n3} x3 detections within the score error of the threshold')
    assert n3 > 0 and n16 > 0 and matched > 0
    assert near <= 0.05 * n3, (near, n3)
    assert score_err <= DET_BOUND[backbone][0] and dist <= DET_BOUND[backbone][1], (score_err, dist)


@pytest.mark.parametrize('backbone', ['resnet50', 'mobile0.25'])
def test_default_path_is_x3_and_bit_equal(monkeypatch, backbone):
    """With KEEP_AMD_DETECT_PRECISION unset the loader builds an 'x3' detector whose detections are those of a directly built one."""
    import sys
    import types
    if 'comfy' not in sys.modules:
        comfy, mm = types.ModuleType('comfy'), types.ModuleType('comfy.model_management')
        mm.get_torch_device = lambda: torch.device('cuda')
        mm.unet_offload_device = lambda: torch.device('cpu')
        mm.soft_empty_cache = lambda: None
        cu = types.ModuleType('comfy.utils')
        comfy.model_management, comfy.utils = mm, cu
        monkeypatch.setitem(sys.modules, 'comfy', comfy)
        monkeypatch.setitem(sys.modules, 'comfy.model_management', mm)
        monkeypatch.setitem(sys.modules, 'comfy.utils', cu)
        fpm = types.ModuleType('folder_paths')
        fpm.models_dir = '/nonexistent/models'
        monkeypatch.setitem(sys.modules, 'folder_paths', fpm)
    from comfyui_keep_amd.modules.keep_model_loader import engine_facelib
    monkeypatch.delenv('KEEP_AMD_DETECT_PRECISION', raising=False)
    W = RF.synth_retinaface_state_dict(seed=0, backbone=backbone)

    class Det:
        def state_dict(self):
            return W
    Det.backbone = {'resnet50': 'Resnet50', 'mobile0.25': 'mobilenet0.25'}[backbone]

    class Hp:
        face_parse = None
    h = Hp()
    h.face_detector = Det()
    engine_facelib(h)
    eng = h.face_detector.engine
    assert eng.precision == 'x3'
    eng.to('cuda')
    assert eng.o.mma == L.MMA_X3 and eng.o.blobx1 is None
    seed, thr = DETECT[backbone]
    frames = torch.randint(0, 256, (3, 150, 210, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    got, want = h.face_detector.detect_batch(frames, thr), engine(backbone, 'x3').detect_batch(frames, conf_threshold=thr)
    assert sum(len(d) for d in want) > 0
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
