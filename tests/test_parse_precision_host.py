"""CPU: the host side of ParseNet's opt-in single-fp16 precision ('f16', KEEP_MMA_X1): the loader knob, the engine's precision
strings, the packed hand-over to pool workers and the hi-only weight twin's layout."""
import sys
import types

import numpy as np
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
    cu.ProgressBar = type('ProgressBar', (), {'__init__': lambda self, total: None, 'update': lambda self, n: None})
    cu.tiled_scale = None
    comfy.model_management, comfy.utils = mm, cu
    fp = types.ModuleType('folder_paths')
    fp.models_dir = '/nonexistent/models'
    sys.modules.update({'comfy': comfy, 'comfy.model_management': mm, 'comfy.utils': cu, 'folder_paths': fp})


_comfy_stub()
from comfyui_keep_amd.engine import hiplib as L  # noqa: E402
from comfyui_keep_amd.engine import ops  # noqa: E402
from comfyui_keep_amd.engine import parsenet as PN  # noqa: E402
from comfyui_keep_amd.engine.weights import pack_blob, views  # noqa: E402


X1_HALO = 'conv3x3_halo_x3s_kernel<0, false, true>'      # the x1 instantiations, as keep_conv2d_plan names them


def _sd():
    return PN.synth_parsenet_state_dict(seed=0, in_size=64, out_size=64)


def test_loader_knob_is_parsed_and_unknown_values_raise(monkeypatch):
    from comfyui_keep_amd.modules import keep_model_loader as KL
    assert KL.parse_precision_knob({}) == 'x3'
    for v in ('x3', 'fp32', 'f16'):
        assert KL.parse_precision_knob({'KEEP_AMD_PARSE_PRECISION': v}) == v
    with pytest.raises(ValueError, match='x3, fp32, f16'):
        KL.parse_precision_knob({'KEEP_AMD_PARSE_PRECISION': 'bf16'})

    class Fake:
        def state_dict(self):
            return _sd()

    class Hp:
        face_detector = None
    for env, want in ((None, 'x3'), ('f16', 'f16'), ('fp32', 'fp32')):
        if env is None:
            monkeypatch.delenv('KEEP_AMD_PARSE_PRECISION', raising=False)
        else:
            monkeypatch.setenv('KEEP_AMD_PARSE_PRECISION', env)
        h = Hp()
        h.face_parse = Fake()
        KL.engine_facelib(h)
        assert isinstance(h.face_parse, PN.EngineFaceParse) and h.face_parse.engine.precision == want
    monkeypatch.setenv('KEEP_AMD_PARSE_PRECISION', 'fp16')
    h = Hp()
    h.face_parse = Fake()
    with pytest.raises(ValueError, match='KEEP_AMD_PARSE_PRECISION'):
        KL.engine_facelib(h)


def test_unknown_precision_string_raises():
    with pytest.raises(ValueError, match='nonsense'):
        PN.ParseNetEngine(_sd(), in_size=64, out_size=64, precision='nonsense')
    for ok in PN.PRECISIONS:
        assert PN.ParseNetEngine(_sd(), in_size=64, out_size=64, precision=ok).precision == ok
    assert PN.PRECISIONS == ('x3', 'fp32', 'f16')


def test_packed_round_trip_keeps_f16():
    eng = PN.ParseNetEngine(_sd(), in_size=64, out_size=64, precision='f16')
    packed = eng.packed()
    twin = PN.ParseNetEngine.from_packed(*packed)
    assert twin.precision == 'f16' and (twin.in_size, twin.out_size) == (64, 64)
    assert np.array_equal(twin._blob, eng._blob)
    with pytest.raises(ValueError):
        PN.ParseNetEngine.from_packed(*packed[:4], 'f32')


def test_hi_only_blob_is_fp16_of_scaled_weights_in_the_packed_order():
    """`weight_x3` under KEEP_MMA_X1 (include/keep_hip.h): one fp16 per weight, fp16(w * 2^e), at the fp32 blob's own element offsets --
    a packed [Cout,KH,KW,Cin] tensor keeps its order -- with make_x3_blob's power-of-two scale per tensor."""
    g = torch.Generator().manual_seed(5)
    t = {'a.weight': (torch.randn(64, 3, 3, 32, generator=g) * 0.03).contiguous(), 'a.bias': torch.randn(64, generator=g),
         'b.weight': (torch.randn(32, 3, 3, 64, generator=g) * 7.0).contiguous(), 'rgb.weight': torch.randn(64, 3, 3, 3, generator=g)}
    blob, index = pack_blob(t)
    dev = torch.from_numpy(blob)
    w = views(dev, index)
    names = ['a.weight', 'b.weight']
    bx, table = ops.make_x1_blob(dev, index, w, names)
    assert bx.dtype == torch.int16 and bx.numel() == dev.numel()
    x3, table3 = ops.make_x3_blob(dev, index, w, names)
    assert table == table3                                       # the scale table of the x3 twin, unchanged
    covered = torch.zeros(dev.numel(), dtype=torch.bool)
    for n in names:
        off, shape = index[n]
        sc = ops.x3_scale_for(float(t[n].abs().max()))
        assert sc == 2.0 ** round(np.log2(sc)) and 2.0 ** 13 < float(t[n].abs().max()) * sc <= 2.0 ** 14
        want = (t[n].reshape(-1) * sc).to(torch.float16)
        got = bx[off:off + t[n].numel()].view(torch.float16)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), n
        # element (co, kh, kw, ci) sits where the packed fp32 tensor keeps it
        co, kh, kw, ci = 5, 2, 1, 17
        flat = ((co * 3 + kh) * 3 + kw) * shape[-1] + ci
        assert got[flat] == (t[n][co, kh, kw, ci] * sc).to(torch.float16)
        # the hi half of the x3 twin is the same rounding
        hi = x3[2 * off:2 * (off + t[n].numel())].view(torch.float16).view(-1, 2, 16)[:, 0].reshape(-1)
        assert torch.equal(hi.view(torch.int16), want.view(torch.int16))
        covered[off:off + t[n].numel()] = True
    assert not bx[~covered].any()                                # tensors outside `names` have no twin

    # ParseNet's rule: the twin rides on exact f32 (the engine holds no x3 twin), and carries its own scale table
    assert PN.ParseNetEngine.X1_RULE == dict(flags=0) and PN.ParseNetEngine.X1_BASE == L.MMA_F32
    rule = dict(PN.ParseNetEngine.X1_RULE, base=PN.ParseNetEngine.X1_BASE)
    o = ops.Ops()
    o.set_precision(L.MMA_F32, dev, None)
    o.set_x1_twin(bx, table, **rule)
    assert o.mma == L.MMA_F32 and o.blobx3 is None and o.x1_flags == 0
    off, _ = index['b.weight']
    assert o.x1_twin(w['b.weight']).data_ptr() == bx[off:].data_ptr() and o.x1_twin(w['b.weight']).numel() == w['b.weight'].numel()
    assert o.x1_twin(w['rgb.weight']) is None and o.x3_twin(w['b.weight']) is None      # a tensor without a twin stays on the base
    assert o.x1_twin(torch.zeros(64, 3, 3, 32)) is None                                      # ... and so does a view outside the packed blob
    assert o._x1_of(w['a.weight'])[1] == 1.0 / ops.x3_scale_for(float(t['a.weight'].abs().max()))
    assert o._x1_of(w['b.weight'][8:24])[1] == 1.0 / ops.x3_scale_for(float(t['b.weight'].abs().max()))      # a row slice: its tensor's scale
    o.set_precision(L.MMA_F32, dev, None)
    assert o.blobx1 is None and o.x1_twin(w['b.weight']) is None                            # a policy change drops the twin
    o.set_precision(L.MMA_X3, dev, None, x3, 1.0, x3_scales=table3)
    with pytest.raises(ValueError, match='fp32 policy'):                                    # the twin's stated base is not this Ops'
        o.set_x1_twin(bx, table, **rule)
    # x3_twin / x3_scale_of on an x3 Ops: two int16 per weight at twice the offset, the tensor's own scale
    assert o.x3_twin(w['b.weight']).data_ptr() == x3[2 * off:].data_ptr() and o.x3_twin(w['b.weight']).numel() == 2 * w['b.weight'].numel()
    assert o.x3_twin(w['rgb.weight']) is None
    assert o.x3_scale_of(w['a.weight']) == 1.0 / ops.x3_scale_for(float(t['a.weight'].abs().max()))
    with pytest.raises(RuntimeError, match='x3 blob'):
        o.x3_scale_of(w['a.bias'])
    for bad in (7, L.MMA_X1):
        with pytest.raises(ValueError):
            o.set_precision(bad)


def test_library_refuses_x1_where_no_kernel_exists():
    """keep_conv2d_plan (host code, no device): KEEP_MMA_X1 plans onto the x1 instantiations of ParseNet's two kernel families and is
    refused with keep_last_error text everywhere else -- GEMM form, prologue, depth not a multiple of 32, 16-wide tiles, no twin."""
    L.load(check_device=False)
    buf = torch.zeros(64, dtype=torch.float32)
    ptr = buf.data_ptr() // 16 * 16 + 16

    def plan(**kw):
        base = dict(N=2, H=64, W=64, Cin=64, Cout=64, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=64, Wo=64, in_ld=64, out_ld=64,
                    mma=L.MMA_X1, inp=ptr, out=ptr, weight=ptr, weight_x3=ptr, x3_acc_scale=1.0, pad_mode=L.PAD_REFLECT)
        base.update(kw)
        return L.conv2d_plan(L.conv_args(**base))
    assert plan().kernel.decode() == X1_HALO and plan().out_amax_ok == 1 and plan().split_k == 1
    assert plan(H=32, W=32, upsample=1).kernel.decode() == X1_HALO
    assert plan(Cout=32).kernel.decode() == X1_HALO
    assert plan(stride=2, Ho=32, Wo=32, Cout=128, out_ld=128).kernel.decode() == 'conv_x3_kernel<2, 2, 2, 2, true, 0, 0, 1, 0, 1>'
    # the same tile rule as x3: the plan follows the reference batch, never N
    assert plan(N=1, stride=2, Ho=32, Wo=32, Cout=128, out_ld=128).kernel.decode() == plan(N=16, stride=2, Ho=32, Wo=32, Cout=128, out_ld=128).kernel.decode()
    for bad in (dict(KH=1, KW=1, pad_t=0, pad_l=0, pad_mode=L.PAD_ZERO),          # GEMM form
                dict(pro_scale=ptr, pro_shift=ptr), dict(pro_act=L.PRO_RELU),      # prologue
                dict(Cin=48, in_ld=48), dict(H=16, W=16, Ho=16, Wo=16),             # depth, 16-wide tiles
                dict(weight_x3=None), dict(split_k=2), dict(upsample=L.UPSAMPLE_X2_PHASES, pad_mode=L.PAD_ZERO)):
        with pytest.raises(L.KeepHipError, match='keep_conv2d'):
            plan(**bad)
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1'):
        plan(Cin=48, in_ld=48)
