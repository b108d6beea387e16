"""CPU: the one single-fp16 substitution rule of ``Ops`` (``Ops._route``) under its three users -- ``_x1_route`` (the blob twin of a convolution:
the base 'f16' of the four engines and GMFlow's knob), ``_up2_x1_route`` (the hi-only phase twin of an Upsample convolution) and ``_attn_x1_route`` (GMFlow's
window attention) -- and the return code that tells the library's refusal from an error (``KeepHipError.code``)."""
import os
import types

import pytest
import torch

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import net as N
from comfyui_keep_amd.engine import ops
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ('_x1_route', '_up2_x1_route', '_attn_x1_route')      # the three users' caches, by attribute


def _ops():
    """An Ops on the x3 policy with KeepNet's 'f16' twin attached (restricted to the streaming 3x3 kernel) and both knobs' rules on."""
    o = ops.Ops()
    o.set_precision(L.MMA_X3, torch.zeros(64), None, torch.zeros(128, dtype=torch.int16))
    o.set_x1_twin(torch.zeros(64, dtype=torch.int16), [(0, 64, 1.0)], flags=0, base_kernel=ops.X3_STREAM_KERNEL)
    o.attn_x1 = o.up2_x1 = True
    return o


@pytest.mark.parametrize('rule', RULES)
def test_route_asks_once_per_key_and_only_eunsup_means_the_base(rule):
    o = _ops()
    routes = getattr(o, rule)
    assert all(getattr(o, r) == {} for r in RULES)
    asked = []
    x1 = True if rule == '_attn_x1_route' else types.SimpleNamespace(kernel='conv3x3_halo_x3s_kernel<1, true, true>', split_k=1)

    def admits():
        asked.append('yes')
        return x1

    def refuses():
        asked.append('no')
        raise L.KeepHipError('keep_conv2d_plan failed (code -2): keep_conv2d: KEEP_MMA_X1 has no kernel for this call', code=L.EUNSUP)

    def broken():
        raise L.KeepHipError('keep_conv2d_plan failed (code -1): keep_conv2d: bad mma 7', code=L.EINVAL)
    assert o._route(routes, 'a', admits) is x1 and o._route(routes, 'a', admits) is x1
    assert o._route(routes, 'b', refuses) is False and o._route(routes, 'b', refuses) is False      # KEEP_EUNSUP: the call stays on the base
    # one query per key: the answers, the refusal included, are cached
    assert o._route(routes, 'a', refuses) is x1 and o._route(routes, 'b', admits) is False and asked == ['yes', 'no']
    assert routes == {'a': x1, 'b': False} and all(getattr(o, r) == {} for r in RULES if r != rule)
    with pytest.raises(L.KeepHipError, match='bad mma'):      # an error is not an answer, and nothing is remembered of it
        o._route(routes, 'c', broken)
    assert 'c' not in routes
    assert o._route(routes, 'c', admits) is x1


@pytest.mark.parametrize('rule', RULES)
def test_route_reads_the_code_and_never_the_text(rule):
    o = _ops()
    routes = getattr(o, rule)

    def looks_refused():
        raise L.KeepHipError('keep_conv2d_plan failed (code -2): the text of a refusal, the code of an error', code=L.EINVAL)

    def looks_broken():
        raise L.KeepHipError('no code in this text', code=L.EUNSUP)

    def no_code():
        raise L.KeepHipError('libkeep_hip.so not found (code -2)')
    for q in (looks_refused, no_code):
        with pytest.raises(L.KeepHipError):
            o._route(routes, 'a', q)
        assert routes == {}
    assert o._route(routes, 'a', looks_broken) is False and routes == {'a': False}


def test_reattaching_the_twin_forgets_the_blob_twin_routes_and_a_policy_change_forgets_all():
    o = _ops()
    for rule in RULES:
        o._route(getattr(o, rule), 'k', lambda: True)
    o.set_x1_twin()                                     # detaching (what set_precision does) forgets the routes of the twin that left
    assert (o._x1_route, o._up2_x1_route, o._attn_x1_route) == ({}, {'k': True}, {'k': True})
    called = []
    assert o._route(o._x1_route, 'k', lambda: called.append(1) or 'again') == 'again' and called == [1]
    o.set_precision(L.MMA_X3, o.blob32, None, o.blobx3, 1.0)      # a policy change forgets them all; the knobs stay as they are set
    assert all(getattr(o, r) == {} for r in RULES) and o.up2_x1 is True and o.attn_x1 is True
    assert ops.Ops().attn_x1 is False and ops.Ops().up2_x1 is False


# ------------------------------------------------------------------------------------------------ the base-plan restriction of 'x1', through conv()
def _conv_with_base_plan(monkeypatch, base_kernel, kernel, split_k=1):
    """Ops.conv on CPU tensors against a stubbed library whose base plan is (kernel, split_k) and which admits every X1 query: returns
    (number of X1 plan queries, the launches' mma, the Ops)."""
    blob = torch.zeros(64 * 9 * 32)
    o = ops.Ops()
    assert o.x1_base_kernel is None and o.x1_base == L.MMA_X3
    o.set_precision(L.MMA_X3, blob, None, torch.zeros(2 * blob.numel(), dtype=torch.int16), 1.0)
    o.set_x1_twin(torch.zeros(blob.numel(), dtype=torch.int16), [(0, blob.numel(), 1.0)], flags=0, base_kernel=base_kernel)
    asked, launches = [], []

    def plan(a):
        if a.mma == L.MMA_X1:
            asked.append(1)
        return types.SimpleNamespace(split_k=1 if a.mma == L.MMA_X1 else split_k, workspace_bytes=0, stats_P=0, wants_bf16_input=0, out_bf16_ok=0,
                                     out_amax_ok=0, kernel=(b'the x1 kernel' if a.mma == L.MMA_X1 else kernel.encode()))
    monkeypatch.setattr(ops, '_PLAN_CACHE', {})
    monkeypatch.setattr(L, 'conv2d_plan', plan)
    monkeypatch.setattr(L, 'conv2d_launch', lambda a: launches.append(a.mma))
    x = torch.zeros(1, 8, 8, 32)
    for _ in range(3):
        o.conv(x, blob.view(64, 3, 3, 32), None, bounded=True)
    return len(asked), launches, o


OTHER_PLANS = [('gemm_x3l_kernel<4>', 1), ('conv_x3_kernel<2, 2, 2, 2, true, true>', 1), ('conv3x3_halo_x3_kernel<32, x2 phases>', 1),
               ('conv3x3_halo_x3_kernel<16>', 1), (ops.X3_STREAM_KERNEL, 4)]


OTHER_IDS = ['gemm_latency', 'gemm_tile', 'up2_phases', 'halo16', 'stream_split4']


@pytest.mark.parametrize('kernel,split_k', OTHER_PLANS, ids=OTHER_IDS)
def test_restricted_rule_does_not_even_ask_about_another_base_plan(monkeypatch, kernel, split_k):
    """KeepNet's rule (base_kernel=X3_STREAM_KERNEL): only the un-split streaming 3x3 kernel is substituted."""
    asked, launches, o = _conv_with_base_plan(monkeypatch, ops.X3_STREAM_KERNEL, kernel, split_k)
    assert asked == 0 and launches == [L.MMA_X3] * 3 and not any(o._x1_route.values())


@pytest.mark.parametrize('base_kernel,kernel,split_k', [(ops.X3_STREAM_KERNEL, ops.X3_STREAM_KERNEL, 1)] + [(None, k, s) for k, s in OTHER_PLANS],
                         ids=['restricted-stream'] + ['unrestricted-' + i for i in OTHER_IDS])
def test_admitted_base_plan_is_asked_once_and_substituted(monkeypatch, base_kernel, kernel, split_k):
    """The restricted rule on its own kernel, and the detectors' rule (no restriction): whatever the base plan is, the library's X1 plan decides."""
    asked, launches, o = _conv_with_base_plan(monkeypatch, base_kernel, kernel, split_k)
    assert asked == 1 and launches == [L.MMA_X1] * 3
    assert [p.kernel for p in o._x1_route.values()] == ['the x1 kernel']


# ------------------------------------------------------------------------------------------------ the built library (host C), no device
def _conv_args(**over):
    buf = torch.zeros(64, dtype=torch.float32)
    ptr = buf.data_ptr() // 16 * 16 + 16
    kw = dict(N=2, H=32, W=128, Cin=128, Cout=128, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=64, Wo=256, in_ld=128, out_ld=128,
              mma=L.MMA_X1, upsample=L.UPSAMPLE_X2_PHASES, inp=ptr, out=ptr, weight=ptr, weight_x3=ptr, x3_acc_scale=1.0,
              flags=L.CONV_X1_UP2, pad_mode=L.PAD_ZERO)
    kw.update(over)
    L.load(check_device=False)
    return L.conv_args(**kw), buf


def test_the_code_travels_with_the_error():
    header = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    assert (L.EINVAL, L.EUNSUP) == (-1, -2) and '#define KEEP_EINVAL (-1)' in header and '#define KEEP_EUNSUP (-2)' in header
    assert L.KeepHipError('a library that was not found').code is None
    a, _buf = _conv_args()
    assert L.conv2d_plan(a).kernel.decode() == ops.X1_UP2_KERNEL
    a, _buf = _conv_args(Cin=48, in_ld=48)              # a depth the single-fp16 phase form has no kernel for: a refusal
    with pytest.raises(L.KeepHipError, match=r'\(code -2\)') as e:
        L.conv2d_plan(a)
    assert e.value.code == L.EUNSUP
    a, _buf = _conv_args()
    a.struct_size -= 4                                  # a malformed struct: an error
    with pytest.raises(L.KeepHipError, match=r'\(code -1\)') as e:
        L.conv2d_plan(a)
    assert e.value.code == L.EINVAL
    kw = dict(q=0x10000, k=0x20000, v=0x30000, o=0x40000, B=16, H=1, Lq=256, Lk=256, D=128, Dv=2, scale=0.088, mode=2, img_h=32, img_w=32,
              ksplit=2, shift=8, kv_rot=2, n_img=4, in_dtype=L.F32, q_bs=1024 * 128, q_ts=128, q_hs=0, k_bs=1024 * 256, k_ts=256, k_hs=0,
              v_bs=2048, v_ts=2, v_hs=0, o_bs=1024 * 128, o_ts=128, o_hs=0)
    with pytest.raises(L.KeepHipError, match=r'\(code -2\).*D = Dv = 128') as e:
        L.attention_x1_plan(**kw)
    assert e.value.code == L.EUNSUP
    assert L.attention_x1_plan(**dict(kw, Dv=128, v_bs=1024 * 256, v_ts=256)) > 0


# ------------------------------------------------------------------------------------------------ KeepNet: one table of the twins' bytes
def test_twin_bytes_and_the_unbuilt_deductions_for_every_knob_and_every_built_state(monkeypatch, synth_weights):
    """``twin_bytes`` and what ``clips_per_call`` takes off the free memory for twins still to be built, against the arithmetic written out
    per knob: 2 / 4 / 6 bytes per blob element for bf16 / x3 / f16, 2 more for the flow twin and the phase twins' bytes on an x3-grade base;
    unbuilt, the x1, flow and phase twins are taken off -- and with an unbuilt x1 twin an unbuilt x3 twin too, with the phase twins once more."""
    import itertools
    for k in ('KEEP_AMD_PRECISION', 'KEEP_AMD_FLOW_PRECISION', 'KEEP_AMD_UPSAMPLE_PRECISION'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('KEEP_AMD_MAX_CLIPS', str(10 ** 9))
    net = N.KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth_weights, strict=True)
    n = int(net._blob.size)
    up = sum(8 * s[0] * s[1] * s[2] * s[3] for s in (net._index[m][1] for m in net.up2_x1_names()))
    assert n > 0 and up > 0
    built = object()
    for prec, flow, ups in itertools.product(N.PRECISIONS, N.FLOW_PRECISIONS, N.UPSAMPLE_PRECISIONS):
        net.set_precision(prec).set_flow_precision(flow).set_upsample_precision(ups)
        for p in N.PRECISIONS:
            grade = p in ('x3', 'f16')
            assert net.twin_bytes(p) == ({'fp32': 0, 'bf16': 2 * n, 'x3': 4 * n, 'f16': 6 * n}[p] + (2 * n if grade and flow == 'f16' else 0)
                                         + (up if grade and ups == 'f16' else 0)), (prec, flow, ups, p)
        assert net.twin_bytes() == net.twin_bytes(prec)
        grade = prec in ('x3', 'f16')
        for x3b, x1b, fb, upb in itertools.product((False, True), repeat=4):
            net._dev_blobx3, net._dev_blobx1, net._dev_blobx1f, net.o.up2_x1 = (built if x3b else None), (built if x1b else None), (built if fb else None), upb
            off = 0
            if prec == 'f16' and not x1b:
                off += 2 * n + (0 if x3b else 4 * n + (up if ups == 'f16' else 0))
            if grade and flow == 'f16' and not fb:
                off += 2 * n
            if grade and ups == 'f16' and not upb:
                off += up
            per_frame = {'bf16': 0.17e9, 'fp32': 0.36e9}.get(prec, 0.23e9) * (64 * 64) / (512.0 * 512.0)
            assert net.clips_per_call(1, 64, 64) == max(1, int(0.8 * (64e9 - off) / per_frame)), (prec, flow, ups, x3b, x1b, fb, upb)
