"""CPU: the host side of RetinaFace's opt-in single-fp16 precision ('f16'): the loader knob, the engine's precision strings and the
library's plan for the 1x1 GEMM form of KEEP_MMA_X1 behind the opt-in bit KEEP_CONV_X1_GEMM."""
import sys
import types

import pytest
import torch


def _comfy_stub():
    if 'comfy' in sys.modules:
        return
    comfy = types.ModuleType('comfy')
    mm = types.ModuleType('comfy.model_management')
    mm.get_torch_device = lambda: torch.device('cpu')
    mm.unet_offload_device = lambda: torch.device('cpu')
    mm.soft_empty_cache = lambda: None
    cu = types.ModuleType('comfy.utils')

    class ProgressBar:              # (the stub tests/test_host_logic.py installs: whichever module is collected first provides it)
        last = None

        def __init__(self, total):
            self.total, self.current = total, 0
            ProgressBar.last = self

        def update(self, n):
            self.current += n

    cu.ProgressBar = ProgressBar
    cu.tiled_scale = None
    comfy.model_management, comfy.utils = mm, cu
    fp = types.ModuleType('folder_paths')
    fp.models_dir = '/nonexistent/models'
    sys.modules.update({'comfy': comfy, 'comfy.model_management': mm, 'comfy.utils': cu, 'folder_paths': fp})


_comfy_stub()
from comfyui_keep_amd.engine import hiplib as L  # noqa: E402
from comfyui_keep_amd.engine import ops  # noqa: E402
from comfyui_keep_amd.engine import retinaface as RF  # noqa: E402

X1_GEMM_64 = 'conv_x3_kernel<2, 2, 1, 1, true, 1, 0, 1, 0, 1>'      # the x1 GEMM instantiations, as keep_conv2d_plan names them
X1_GEMM_128 = 'conv_x3_kernel<2, 2, 2, 2, true, 1, 0, 1, 0, 1>'
X1_IM2COL = ('conv_x3_kernel<2, 2, 1, 1, true, 0, 0, 1, 0, 1>', 'conv_x3_kernel<2, 2, 2, 2, true, 0, 0, 1, 0, 1>')


def test_loader_knob_is_parsed_and_unknown_values_raise():
    from comfyui_keep_amd.modules import keep_model_loader as KL
    assert KL.detect_precision_knob({}) == 'x3'
    assert KL.detect_precision_knob({'KEEP_AMD_DETECT_PRECISION': ''}) == 'x3'
    for v in ('x3', 'fp32', 'f16'):
        assert KL.detect_precision_knob({'KEEP_AMD_DETECT_PRECISION': v}) == v
    with pytest.raises(ValueError, match='x3, fp32, f16'):
        KL.detect_precision_knob({'KEEP_AMD_DETECT_PRECISION': 'bf16'})


@pytest.mark.parametrize('backbone', ['resnet50', 'mobile0.25'])
def test_loader_applies_the_knob_to_the_retinaface_engines(monkeypatch, backbone):
    from comfyui_keep_amd.modules import keep_model_loader as KL
    sd = RF.synth_retinaface_state_dict(seed=0, backbone=backbone)

    class Det:
        def state_dict(self):
            return sd
    Det.backbone = {'resnet50': 'Resnet50', 'mobile0.25': 'mobilenet0.25'}[backbone]

    class Hp:
        face_parse = None
    for env, want in ((None, 'x3'), ('f16', 'f16'), ('fp32', 'fp32')):
        if env is None:
            monkeypatch.delenv('KEEP_AMD_DETECT_PRECISION', raising=False)
        else:
            monkeypatch.setenv('KEEP_AMD_DETECT_PRECISION', env)
        h = Hp()
        h.face_detector = Det()
        KL.engine_facelib(h)
        assert isinstance(h.face_detector, RF.EngineRetinaFace) and h.face_detector.engine.precision == want
        assert h.face_detector.engine.backbone == backbone
    monkeypatch.setenv('KEEP_AMD_DETECT_PRECISION', 'fp16')
    h = Hp()
    h.face_detector = Det()
    with pytest.raises(ValueError, match='KEEP_AMD_DETECT_PRECISION'):
        KL.engine_facelib(h)


@pytest.mark.parametrize('backbone', ['resnet50', 'mobile0.25'])
def test_unknown_precision_string_raises(backbone):
    sd = RF.synth_retinaface_state_dict(seed=0, backbone=backbone)
    with pytest.raises(ValueError, match='nonsense'):
        RF.RetinaFaceEngine(sd, precision='nonsense')
    assert RF.RetinaFaceEngine.PRECISIONS == ('x3', 'fp32', 'f16')
    for ok in RF.RetinaFaceEngine.PRECISIONS:
        assert RF.RetinaFaceEngine(sd, precision=ok).precision == ok
    assert RF.EngineRetinaFace(RF.RetinaFaceEngine(sd, precision='f16')).engine.precision == 'f16'


def _planner():
    L.load(check_device=False)
    buf = torch.zeros(64, dtype=torch.float32)
    ptr = buf.data_ptr() // 16 * 16 + 16

    def plan(**kw):
        base = dict(N=2, H=40, W=23, Cin=64, Cout=32, KH=1, KW=1, stride=1, pad_t=0, pad_l=0, Ho=40, Wo=23, in_ld=64, out_ld=32,
                    mma=L.MMA_X1, inp=ptr, out=ptr, weight=ptr, weight_x3=ptr, x3_acc_scale=1.0, flags=L.CONV_X1_GEMM)
        base.update(kw)
        return L.conv2d_plan(L.conv_args(**base))
    return plan, ptr, buf


def test_library_plans_the_x1_gemm_form_behind_the_flag():
    """keep_conv2d_plan (host code, no device): with KEEP_CONV_X1_GEMM a 1x1 stride-1 call plans onto the x1 instantiation of the GEMM
    variant of conv_x3_kernel by the x3 rules -- the same kernel whatever N is; without the bit the call is refused as before."""
    plan, ptr, _buf = _planner()
    assert L.CONV_X1_GEMM == 1 << 14 and L.ABI_VERSION == 23
    assert plan().kernel.decode() == X1_GEMM_64                                       # Cout = 32: the 64 x 64 tile
    big = dict(Cout=256, out_ld=256)
    assert plan(**big).kernel.decode() == X1_GEMM_128                                 # 16 reference images x 920 rows: the 128 x 128 tile
    assert plan(H=8, W=8, Ho=8, Wo=8, **big).kernel.decode() == X1_GEMM_64           # few reference rows: the small tile
    for kw in ({}, big, dict(H=8, W=8, Ho=8, Wo=8, **big)):
        p1, p16 = plan(N=1, **kw), plan(N=16, **kw)
        assert (p1.kernel, p1.split_k) == (p16.kernel, p16.split_k)
    # what the x3 GEMM form allows stays allowed: residual (res_ld), epilogue activation, an out_ld slice
    assert plan(residual=ptr, res_ld=48, epi_act=L.ACT_RELU, out_ld=48).kernel.decode() == X1_GEMM_64
    # a shape the x3 policy sends to the latency form (gemm_x3l_kernel) takes the x1 tile kernel: there is no x1 latency form
    lat = dict(H=16, W=16, Ho=16, Wo=16, Cin=512, in_ld=512, Cout=512, out_ld=512)
    assert plan(mma=L.MMA_X3, **lat).kernel.decode().startswith('gemm_x3l_kernel')
    assert plan(**lat).kernel.decode() in (X1_GEMM_64, X1_GEMM_128)
    # the fused max|out| where a wave's rows lie in one image and the plan is one pass
    assert plan(H=8, W=8, Ho=8, Wo=8).out_amax_ok == 1 and plan().out_amax_ok == 0      # (920 rows per image: not a multiple of 32)
    # the bit does not touch the other x1 forms
    assert plan(KH=3, KW=3, pad_t=1, pad_l=1, H=64, W=64, Ho=64, Wo=64).kernel.decode() == 'conv3x3_halo_x3s_kernel<0, false, true>'
    assert plan(stride=2, Ho=20, Wo=12).kernel.decode() in X1_IM2COL
    # ... and opens the im2col form to the 3x3 stride-1 convolutions no halo kernel tiles (x3 runs the same im2col kernel there)
    ragged = dict(KH=3, KW=3, pad_t=1, pad_l=1)
    assert plan(**ragged).kernel.decode() in X1_IM2COL
    assert plan(mma=L.MMA_X3, **ragged).kernel.decode().startswith('conv_x3_kernel<')
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1'):
        plan(flags=0, **ragged)
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1'):                           # a 16 x 16-tileable map keeps x3's halo kernel
        plan(H=16, W=16, Ho=16, Wo=16, **ragged)


def test_library_refuses_the_x1_gemm_form_where_it_must():
    plan, ptr, _buf = _planner()
    for bad in (dict(Cin=48, in_ld=48), dict(pro_scale=ptr, pro_shift=ptr), dict(pro_act=L.PRO_RELU),
                dict(aux=ptr, residual=ptr, res_ld=32), dict(weight_x3=None), dict(x3_acc_scale=0.0)):
        with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1'):
            plan(**bad)
    # in2 and the LayerNorm epilogue are KEEP_MMA_X3 features: refused before the plan, with the policy named
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X3'):
        plan(in2=ptr, in2_cin1=32, Cin=64, in_ld=32)
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X3'):
        plan(ln_gamma=ptr, ln_beta=ptr, Cout=128, out_ld=128)
    # without the bit: refused exactly as before
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1 has no kernel for this call: it needs weight_x3'):
        plan(flags=0)
    with pytest.raises(L.KeepHipError, match='not a 1x1 GEMM'):
        plan(flags=0, Cout=256, out_ld=256)
    # the bit is ignored by the other policies
    for mma in (L.MMA_X3, L.MMA_F32):
        a, b = plan(mma=mma), plan(mma=mma, flags=0)
        assert (a.kernel, a.split_k, a.path) == (b.kernel, b.split_k, b.path)
