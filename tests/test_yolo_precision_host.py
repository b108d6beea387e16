"""CPU: the host side of YOLOv5-face's opt-in single-fp16 precision ('f16'): the engine's precision strings, the loader knob reaching
``EngineYoloModel.from_module``, and the library's plan for the 16 x 16-tile single-fp16 halo form behind KEEP_CONV_X1_HALO16
(keep_conv2d_plan is host code: no device)."""
import pytest
import torch

import test_detect_precision_host as _stub      # noqa: F401  (installs the comfy / folder_paths stubs the loader module imports)
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops
from comfyui_keep_amd.engine import yoloface as YF

X1_HALO16 = 'conv3x3_halo_x3_kernel<16, 0, true, true, true, false, true>'        # <TW, PRO, SIMPLE_EPI, FASTACT, WDMA, UP2, X1>
X1_HALO16_ACT = 'conv3x3_halo_x3_kernel<16, 0, false, true, true, false, true>'   # an epilogue activation: the general epilogue
X1_STREAM = 'conv3x3_halo_x3s_kernel<0, false, true>'
BOTH = L.CONV_X1_GEMM | L.CONV_X1_HALO16


@pytest.mark.parametrize('name', ['YOLOv5n', 'YOLOv5l'])
def test_unknown_precision_string_raises(name):
    sd = YF.synth_yolo_state_dict(name, seed=0)
    assert YF.YoloFaceEngine.PRECISIONS == ('x3', 'fp32', 'f16')
    with pytest.raises(ValueError, match='bogus'):
        YF.YoloFaceEngine(sd, precision='bogus')
    for ok in YF.YoloFaceEngine.PRECISIONS:
        assert YF.YoloFaceEngine(sd, precision=ok).precision == ok


def test_loader_hands_the_knob_to_the_yolo_engine(monkeypatch):
    from comfyui_keep_amd.modules import keep_model_loader as KL
    sd = YF.synth_yolo_state_dict('YOLOv5n', seed=0)

    class Net:
        def state_dict(self):
            return sd

    class Det:
        pass

    class Hp:
        face_parse = None
    seen = []
    real = YF.EngineYoloModel.from_module.__func__

    def spy(cls, module, device=None, precision='x3'):
        seen.append(precision)
        return real(cls, module, device=device, precision=precision)
    monkeypatch.setattr(YF.EngineYoloModel, 'from_module', classmethod(spy))
    for env, want in ((None, 'x3'), ('f16', 'f16'), ('fp32', 'fp32')):
        if env is None:
            monkeypatch.delenv('KEEP_AMD_DETECT_PRECISION', raising=False)
        else:
            monkeypatch.setenv('KEEP_AMD_DETECT_PRECISION', env)
        h = Hp()
        h.face_detector = Det()
        h.face_detector.detector = Net()
        KL.engine_facelib(h)
        assert seen[-1] == want
        assert isinstance(h.face_detector.detector, YF.EngineYoloModel) and h.face_detector.detector.engine.precision == want
    assert not hasattr(KL, '_yolo_f16_warned')
    monkeypatch.setenv('KEEP_AMD_DETECT_PRECISION', 'half')
    h = Hp()
    h.face_detector = Det()
    h.face_detector.detector = Net()
    with pytest.raises(ValueError, match='KEEP_AMD_DETECT_PRECISION'):
        KL.engine_facelib(h)


def test_twin_flags_default_leaves_the_gemm_bit_alone():
    from comfyui_keep_amd.engine import retinaface as RF
    o = ops.Ops()
    assert o.x1_flags == L.CONV_X1_GEMM
    o.set_x1_twin(None, None)
    assert o.x1_flags == L.CONV_X1_GEMM                  # RetinaFace's call: unchanged
    o.set_x1_twin(None, None, flags=BOTH)
    assert o.x1_flags == BOTH
    o.set_precision(L.MMA_F32)
    assert o.x1_flags == L.CONV_X1_GEMM and o.x1_base_kernel is None and o.x1_base == L.MMA_X3
    assert RF.RetinaFaceEngine.X1_RULE == dict(flags=L.CONV_X1_GEMM) and YF.YoloFaceEngine.X1_RULE == dict(flags=BOTH)


def _planner():
    L.load(check_device=False)
    buf = torch.zeros(64, dtype=torch.float32)
    ptr = buf.data_ptr() // 16 * 16 + 16

    def plan(**kw):
        base = dict(N=2, H=16, W=16, Cin=64, Cout=128, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=16, Wo=16, in_ld=64, out_ld=128,
                    mma=L.MMA_X1, inp=ptr, out=ptr, weight=ptr, weight_x3=ptr, x3_acc_scale=1.0, flags=L.CONV_X1_HALO16, plan_ref_images=128)
        base.update(kw)
        return L.conv2d_plan(L.conv_args(**base))
    return plan, ptr, buf


def test_library_plans_the_x1_halo16_form_behind_the_flag():
    """A 3x3 stride-1 pad-1 Cin = 64 call on a 16 x 16 and on a 48 x 80 map.  The form is admitted only where KEEP_MMA_X3 plans the same call
    un-split: 128 reference images x one 256-pixel tile x two 64-cout blocks = 256 items on the 16 x 16 map (what a caller with the default
    16 reference images gets on the 48 x 80 map of a 768 x 1280 letterbox: 16 x 15 x 2 = 480 here)."""
    plan, ptr, _buf = _planner()
    assert L.CONV_X1_HALO16 == 1 << 15 and L.ABI_VERSION == 23
    big = dict(H=48, W=80, Ho=48, Wo=80, plan_ref_images=0)
    for kw in ({}, big):
        pl = plan(**kw)
        assert pl.kernel.decode() == X1_HALO16 and pl.split_k == 1 and pl.workspace_bytes == 0 and pl.out_amax_ok == 1, kw
        assert plan(mma=L.MMA_X3, **kw).kernel.decode() == 'conv3x3_halo_x3_kernel<16>' and plan(mma=L.MMA_X3, **kw).split_k == 1
        assert plan(flags=BOTH, **kw).kernel.decode() == X1_HALO16
        p1, p16 = plan(N=1, **kw), plan(N=16, **kw)
        assert (p1.kernel, p1.split_k) == (p16.kernel, p16.split_k)                  # planned from plan_ref_images, never from N
    assert plan(epi_act=L.ACT_SILU).kernel.decode() == X1_HALO16_ACT
    assert plan(residual=ptr, res_ld=256, out_ld=256, bias=ptr).kernel.decode() == X1_HALO16
    assert plan(Cout=48, out_ld=48, plan_ref_images=256).kernel.decode() == X1_HALO16   # Cout in float4 groups, not whole 64-cout blocks
    # without the bit the same calls are refused with the texts they always had
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1 has no kernel for this call: it needs weight_x3'):
        plan(flags=0)
    with pytest.raises(L.KeepHipError, match='not a 1x1 GEMM'):
        plan(flags=0, **big)
    with pytest.raises(L.KeepHipError, match=r'KEEP_MMA_X1 \(with KEEP_CONV_X1_GEMM\) has no kernel for this call'):
        plan(flags=L.CONV_X1_GEMM)


def test_library_refuses_the_x1_halo16_form_where_it_must():
    plan, ptr, _buf = _planner()
    # a map of 8 x 32 tiles keeps the streaming form (with or without the bit)
    wide = dict(H=32, W=32, Ho=32, Wo=32)
    assert plan(**wide).kernel.decode() == X1_STREAM and plan(flags=0, **wide).kernel.decode() == X1_STREAM
    for bad in (dict(pro_scale=ptr, pro_shift=ptr), dict(pro_act=L.PRO_RELU), dict(Cin=48, in_ld=48), dict(pad_mode=L.PAD_REFLECT),
                dict(aux=ptr, residual=ptr, res_ld=128), dict(weight_x3=None), dict(x3_acc_scale=0.0), dict(H=8, W=8, upsample=1),
                dict(H=24, W=24, Ho=24, Wo=24)):
        with pytest.raises(L.KeepHipError, match='KEEP_CONV_X1_HALO16'):
            plan(**bad)
    # a call KEEP_MMA_X3 would split stays x3: one reference image, Cout = 64 -> one item, K split two ways
    split = dict(plan_ref_images=1, Cout=64, out_ld=64)
    assert plan(mma=L.MMA_X3, **split).split_k == 2
    with pytest.raises(L.KeepHipError, match='split-K = 2'):
        plan(**split)
    with pytest.raises(L.KeepHipError, match='split-K = 4'):                      # ... or one the caller splits
        plan(split_k=4)
    with pytest.raises(L.KeepHipError, match='split-K'):                          # the default 16 reference images on a 16 x 16 map: 32 items
        plan(plan_ref_images=0)
    # the bit is ignored by the other policies
    for mma in (L.MMA_X3, L.MMA_F32):
        a, b = plan(mma=mma), plan(mma=mma, flags=0)
        assert (a.kernel, a.split_k, a.path) == (b.kernel, b.split_k, b.path)
