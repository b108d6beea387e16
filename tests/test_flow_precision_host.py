"""CPU: the host side of GMFlow's opt-in single-fp16 precision (KEEP_AMD_FLOW_PRECISION=f16) -- the knob, the flow twin's name list, the
attention routing rule of Ops (``attn_x1``), and what the built library answers to KEEP_MMA_X1 | KEEP_ATTN_X1 without a device."""
import ctypes

import pytest
import torch

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import net as N
from comfyui_keep_amd.engine import ops
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH

KNOB = 'KEEP_AMD_FLOW_PRECISION'


def test_knob_parsing(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    assert N.KeepNet(**DEFAULT_ARCH).flow_precision == 'x3'
    for v in ('x3', 'f16'):
        monkeypatch.setenv(KNOB, v)
        assert N.KeepNet(**DEFAULT_ARCH).flow_precision == v
    monkeypatch.setenv(KNOB, 'fp16')
    with pytest.raises(ValueError, match=KNOB):
        N.KeepNet(**DEFAULT_ARCH)
    monkeypatch.delenv(KNOB)
    net = N.KeepNet(**DEFAULT_ARCH)
    assert net.set_flow_precision('f16').flow_precision == 'f16' and net.set_flow_precision('x3').flow_precision == 'x3'
    with pytest.raises(ValueError, match=KNOB):
        net.set_flow_precision('bf16')
    assert N.FLOW_PRECISIONS == ('x3', 'f16') and N.PRECISIONS == ('fp32', 'x3', 'bf16', 'f16')      # the base tuple is untouched


@pytest.mark.parametrize('base', ['fp32', 'bf16'])
def test_flow_f16_needs_an_x3_grade_base(base, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    net = N.KeepNet(**DEFAULT_ARCH).set_precision(base).set_flow_precision('f16')
    with pytest.raises(ValueError, match=KNOB):
        net._activate_flow_precision()
    net.set_flow_precision('x3')._activate_flow_precision()      # the knob off: nothing to refuse, and no second Ops
    assert net.of is net.o


def test_knob_off_is_the_same_ops_object(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    net = N.KeepNet(**DEFAULT_ARCH)
    assert net.of is net.o and net._of is None
    net._activate_flow_precision()
    assert net.of is net.o and net._of is None and net.o.attn_x1 is False
    n = 1000
    net._blob = torch.zeros(n).numpy()
    assert net.twin_bytes('x3') == 4 * n and net.twin_bytes('f16') == 6 * n
    net.set_flow_precision('f16')      # the flow twin is counted: 2 bytes per blob element on either x3-grade base
    assert net.twin_bytes('x3') == 6 * n and net.twin_bytes('f16') == 8 * n and net.twin_bytes('bf16') == 2 * n
    assert net.pool_config()['flow_precision'] == 'f16'


def test_flow_twin_names(synth_weights):
    net = N.KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth_weights, strict=True)
    idx = net._index
    flow, base = N.KeepNet.flow_x1_names(idx), N.KeepNet.x1_names(idx)
    assert flow and all(n.startswith('flownet.') for n in flow) and not set(flow) & set(base)
    for n in flow:
        shape = idx[n][1]
        assert shape[-1] % 32 == 0 and (len(shape) == 2 or (len(shape) == 4 and tuple(shape[1:3]) == (3, 3))), (n, shape)
    # every kind is there: the backbone's 3x3 and 1x1 convolutions, the swin projections, the flow-propagation projections
    for must in ('flownet.model.backbone.layer1.0.conv1.weight', 'flownet.model.backbone.layer2.0.conv1.weight', 'flownet.model.backbone.conv2.weight',
                 'flownet.model.transformer.layers.0.self_attn.qkv.weight', 'flownet.model.transformer.layers.0.self_attn.merge.weight',
                 'flownet.model.feature_flow_attn.q_proj.weight', 'flownet.model.feature_flow_attn.k_proj.weight'):
        assert must in flow, must
    # the 16-channel s2d stem and the RGB stem have no twin: they stay on the base policy
    assert not any('backbone.conv1.' in n for n in flow)
    # everything left out of the twin has Cin % 32 != 0, is no matrix weight, is neither 3x3 nor 1x1 / linear -- or is one of the two
    # stride-2 1x1 shortcut convolutions, which measured no faster under single fp16 and stay x3
    left = [n for n in idx if n.startswith('flownet.') and n not in flow]
    for n in left:
        shape = idx[n][1]
        assert len(shape) < 2 or shape[-1] % 32 or (len(shape) == 4 and tuple(shape[1:3]) != (3, 3)) or '.downsample.0.weight' in n, (n, shape)
    assert sorted(n for n in left if '.downsample.0.weight' in n) == ['flownet.model.backbone.layer2.0.downsample.0.weight',
                                                                     'flownet.model.backbone.layer3.0.downsample.0.weight']


def _attention_through_a_stub(monkeypatch, o, Dv=128, **over):
    """Ops.attention on CPU tensors with the binding's two entry points replaced: returns (plan queries, launches as (mma, flags))."""
    plans, launches = [], []

    def plan(**kw):
        plans.append((kw['Lq'], kw['Dv']))
        if kw['Dv'] != 128:
            raise L.KeepHipError('keep_attention plan failed (code -2): keep_attention: KEEP_MMA_X1 covers D = Dv = 128 only', code=L.EUNSUP)
        return 4096

    monkeypatch.setattr(L, 'attention_x1_plan', plan)
    monkeypatch.setattr(L, 'attention', lambda **kw: launches.append((kw['mma'], kw['flags'])))
    q = torch.zeros(2 * 256, 128)
    v = torch.zeros(2 * 256, Dv)
    kw = dict(B=2, H=1, Lq=256, Lk=256, D=128, Dv=Dv, scale=1.0, q_str=(256 * 128, 128, 0), k_str=(256 * 128, 128, 0), v_str=(256 * Dv, Dv, 0),
              o_str=(256 * Dv, Dv, 0))
    kw.update(over)
    for _ in range(3):
        o.attention(q, q, v, torch.empty_like(v), **kw)
    return plans, launches


def test_ops_attention_rule_with_a_stub_library(monkeypatch):
    o = ops.Ops()
    o.mma = o.attn_mma = L.MMA_X3
    o.attn_flags = L.ATTN_NO_SMALL
    # the rule is off by default: not a single X1 query, every launch is the base's
    plans, launches = _attention_through_a_stub(monkeypatch, o)
    assert plans == [] and launches == [(L.MMA_X3, L.ATTN_NO_SMALL)] * 3
    o.attn_x1 = True
    plans, launches = _attention_through_a_stub(monkeypatch, o)
    assert plans == [(256, 128)] and launches == [(L.MMA_X1, L.ATTN_NO_SMALL | L.ATTN_X1)] * 3      # one query per shape key, x1 where admitted
    plans, launches = _attention_through_a_stub(monkeypatch, o, Dv=2)
    assert plans == [(256, 2)] and launches == [(L.MMA_X3, L.ATTN_NO_SMALL)] * 3                     # KEEP_EUNSUP: the call stays on x3
    assert list(o._attn_x1_route.values()) == [True, False]
    plans, launches = _attention_through_a_stub(monkeypatch, o, B=7)                                  # the batch is no part of the key
    assert plans == [] and launches == [(L.MMA_X1, L.ATTN_NO_SMALL | L.ATTN_X1)] * 3
    # an explicit policy of another kind, or another base, is never asked about
    plans, launches = _attention_through_a_stub(monkeypatch, o, mma=L.MMA_F32)
    assert plans == [] and launches == [(L.MMA_F32, L.ATTN_NO_SMALL)] * 3
    o.attn_mma = L.MMA_BF16
    plans, launches = _attention_through_a_stub(monkeypatch, o)
    assert plans == [] and launches == [(L.MMA_BF16, L.ATTN_NO_SMALL)] * 3
    # any other error of the query propagates
    o.attn_mma = L.MMA_X3

    def broken(**kw):
        raise L.KeepHipError('keep_attention plan failed (code -3): hip error', code=-3)
    monkeypatch.setattr(L, 'attention_x1_plan', broken)
    q = torch.zeros(512, 128)
    with pytest.raises(L.KeepHipError, match='code -3'):
        o.attention(q, q, q, torch.empty_like(q), B=1, H=1, Lq=512, Lk=512, D=128, Dv=128, scale=1.0, q_str=(512 * 128, 128, 0), k_str=(512 * 128, 128, 0),
                    v_str=(512 * 128, 128, 0), o_str=(512 * 128, 128, 0))


# ------------------------------------------------------------------------------------------------ the built library, no device
def _args(**over):
    """The 256-token window call of GMFlow at 256 x 256 (mode 2, D = Dv = 128): only shapes and alignment enter the plan."""
    kw = dict(q=0x10000, k=0x20000, v=0x30000, o=0x40000, B=16, H=1, Lq=256, Lk=256, D=128, Dv=128, scale=0.088, mode=2, img_h=32, img_w=32,
              ksplit=2, shift=8, kv_rot=2, n_img=4, in_dtype=L.F32, mma=L.MMA_X1, flags=L.ATTN_X1,
              q_bs=1024 * 128, q_ts=128, q_hs=0, k_bs=1024 * 256, k_ts=256, k_hs=0, v_bs=1024 * 256, v_ts=256, v_hs=0, o_bs=1024 * 128, o_ts=128, o_hs=0)
    kw.update(over)
    return L.attn_args(**kw)


def _last_error():
    return L.load(check_device=False).keep_last_error().decode()


def test_workspace_of_the_flagged_call_is_the_documented_formula():
    for B, Lk, extra in ((16, 256, {}), (2, 300, dict(mode=0, Lq=288, Lk=300, B=2))):
        x1 = L.attention_workspace_bytes(_args(**extra))
        x3 = L.attention_workspace_bytes(_args(mma=L.MMA_X3, flags=0, **extra))
        tiles = (Lk + 31) // 32
        assert x1 == B * 1 * tiles * (32 * (128 + 8) + 128 * 40) * 2, (x1, B, Lk)
        assert x3 == B * 1 * tiles * (32 * (2 * 128 + 8) + 128 * 72) * 2 and 0 < x1 < x3
        assert L.attention_x1_plan(**{f: getattr(_args(**extra), f) for f, _ in L.AttnArgs._fields_ if f not in ('struct_size',)}) == x1
    # every other policy ignores the bit
    assert L.attention_workspace_bytes(_args(mma=L.MMA_X3)) == L.attention_workspace_bytes(_args(mma=L.MMA_X3, flags=0))
    assert L.attention_workspace_bytes(_args(mma=L.MMA_F32)) == 0 and L.attention_workspace_bytes(_args(mma=L.MMA_BF16)) == 0


@pytest.mark.parametrize('what,over,text', [
    ('another head size', dict(D=64), 'D = Dv = 128'),
    ('another value width', dict(Dv=2, v_ts=2, v_bs=2048), 'D = Dv = 128'),
    ('few queries', dict(mode=0, Lq=128, Lk=256), 'Lq'),
    ('sparse-causal keys', dict(mode=1, T=2, seg_len=128), 'mode'),
    ('range probes', dict(mode=0, q_amax=0x1000, k_amax=0x1000, v_amax=0x1000), 'amax'),
    ('bf16 inputs', dict(in_dtype=L.BF16), 'fp32'),
    ('unaligned rows', dict(k_ts=258), '16-byte'),
    ('unaligned base', dict(v=0x30004), '16-byte'),
    ('KEEP_ATTN_NO_PACK', dict(flags=L.ATTN_X1 | L.ATTN_NO_PACK), 'KEEP_ATTN_NO_PACK'),
])
def test_the_flagged_call_refuses_everything_else(what, over, text):
    lib = L.load(check_device=False)
    a = _args(**over)
    assert L.attention_workspace_bytes(a) == -1, what
    assert text in _last_error() and 'KEEP_MMA_X1' in _last_error(), (what, _last_error())
    # keep_attention itself: KEEP_EUNSUP at plan time, before anything touches the device (the pointers are never read)
    assert lib.keep_attention(ctypes.byref(a), None) == -2, what
    assert text in _last_error(), (what, _last_error())
    with pytest.raises(L.KeepHipError, match=r'\(code -2\)'):
        L.attention_x1_plan(**{f: getattr(a, f) for f, _ in L.AttnArgs._fields_ if f != 'struct_size'})


def test_a_workspace_that_is_too_small_is_refused():
    lib = L.load(check_device=False)
    a = _args()
    need = L.attention_workspace_bytes(a)
    for ws, nbytes in ((None, 0), (0x50000, need - 16), (0x50008, need)):      # none, too small, misaligned
        a.workspace, a.workspace_bytes = ws, nbytes
        assert lib.keep_attention(ctypes.byref(a), None) == -2 and 'workspace' in _last_error() and 'KEEP_MMA_X1' in _last_error(), (ws, nbytes)


def test_x1_without_the_bit_is_still_refused():
    lib = L.load(check_device=False)
    a = _args(flags=0)
    assert L.attention_workspace_bytes(a) == 0
    assert lib.keep_attention(ctypes.byref(a), None) == -1 and 'KEEP_MMA_X1' in _last_error()
    assert L.ATTN_X1 == 1 << 5 and L.ABI_VERSION == 23
