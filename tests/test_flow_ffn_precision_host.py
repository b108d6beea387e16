"""CPU: the host side of the opt-in single-fp16 form of GMFlow's fused feed-forward block (KEEP_AMD_FLOW_FFN_PRECISION=f16) -- the two entry
points keep_gm_ffn_x1 / keep_gm_ffn_x1_plan in the extension header, the binding and the built library (refusals and plan answers are host
C), the KeepNet knob, the routing rule of Ops.gm_ffn against a stubbed library, and the hi-only twin builders against the x3 twins."""
import ctypes
import os
import re

import pytest
import torch

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import net as N
from comfyui_keep_amd.engine import ops
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = 'KEEP_AMD_FLOW_FFN_PRECISION'
NAMES = ('keep_gm_ffn_x1', 'keep_gm_ffn_x1_plan')


# ------------------------------------------------------------------------------------------------ header, binding, library
def test_header_binding_and_library_agree_on_the_two_symbols():
    header = open(os.path.join(ROOT, 'include', 'keep_cv_hip.h')).read()
    core = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    bound = L.load(check_device=False)
    for name in NAMES:
        assert name in L.CV_EXPORTED_SYMBOLS and name in L._CV_SIGNATURES and name not in L.EXPORTED_SYMBOLS
        assert not re.search(r'\b' + name + r'\b', core)                      # the extension header only
        proto = re.search(r'int32_t ' + name + r'\s*\(([^;]*)\);', header).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', proto).split(',')) == len(L._CV_SIGNATURES[name]), name
        assert getattr(bound, name).argtypes == L._CV_SIGNATURES[name] and getattr(bound, name).restype is ctypes.c_int32
    assert L._CV_SIGNATURES['keep_gm_ffn_x1'] == L._SIGNATURES['keep_gm_ffn_x3']      # the x3 entry's argument list
    assert len(L._CV_SIGNATURES['keep_gm_ffn_x1_plan']) == 5
    assert int(re.search(r'#define KEEP_CV_ABI_VERSION (\d+)', header).group(1)) == L.CV_ABI_VERSION == 1
    assert L.ABI_VERSION == 23 and len(L.EXPORTED_SYMBOLS) == 63


_P = 0x10000      # a placeholder device pointer: every refusal below comes before anything is launched or dereferenced


def _launch(**over):
    kw = dict(src=_P, msg=_P, w0=_P, a0=1.0, w2=_P, a2=1.0, g=_P, b=_P, eps=1e-5, out=_P, M=256, C=128, hidden=1024, exact=0)
    kw.update(over)
    lib = L.load(check_device=False)
    rc = lib.keep_gm_ffn_x1(kw['src'], kw['msg'], kw['w0'], kw['a0'], kw['w2'], kw['a2'], kw['g'], kw['b'], kw['eps'], kw['out'], kw['M'], kw['C'],
                            kw['hidden'], kw['exact'], None)
    return rc, lib.keep_last_error().decode()


@pytest.mark.parametrize('what,over', [
    ('null src', dict(src=None)), ('null msg', dict(msg=None)), ('null w0', dict(w0=None)), ('null w2', dict(w2=None)),
    ('null gamma', dict(g=None)), ('null beta', dict(b=None)), ('null out', dict(out=None)),
    ('C != 128', dict(C=64)), ('C != 128 (256)', dict(C=256)), ('hidden % 32', dict(hidden=48)), ('hidden = 0', dict(hidden=0)),
    ('src alignment', dict(src=_P + 4)), ('msg alignment', dict(msg=_P + 8)), ('w0 alignment', dict(w0=_P + 2)), ('w2 alignment', dict(w2=_P + 2)),
    ('out alignment', dict(out=_P + 4)), ('gamma alignment', dict(g=_P + 4)), ('beta alignment', dict(b=_P + 12)),
    ('weights beyond 2 GB', dict(hidden=1 << 23)), ('M = 0', dict(M=0)), ('M < 0', dict(M=-5)),
])
def test_launcher_refusals_come_before_any_launch_and_name_the_function(what, over):
    rc, msg = _launch(**over)
    assert rc == L.EINVAL == -1, (what, rc, msg)
    assert msg.startswith('keep_gm_ffn_x1:'), (what, msg)


def test_plan_answers():
    assert L.gm_ffn_x1_plan(128, 1024) is True and L.gm_ffn_x1_plan(128, 32) is True
    lib = L.load(check_device=False)
    for args, text in (((64, 1024, 0, 0, 0), 'C = 128'), ((128, 48, 0, 0, 0), 'chunks of 32'), ((128, 1024, 4, 0, 0), 'aligned'),
                       ((128, 1024, 0, 2, 0), 'aligned'), ((128, 1024, 0, 0, 8), 'aligned'), ((128, 1 << 23, 0, 0, 0), '2 GB')):
        with pytest.raises(L.KeepHipError) as e:
            L.gm_ffn_x1_plan(*args)
        assert e.value.code == L.EUNSUP == -2 and text in str(e.value), (args, str(e.value))
        assert lib.keep_last_error().decode().startswith('keep_gm_ffn_x1_plan:')
    for args in ((0, 1024, 0, 0, 0), (128, -32, 0, 0, 0), (128, 1024, -1, 0, 0)):      # no shape at all: an error, not 'stay on x3'
        with pytest.raises(L.KeepHipError) as e:
            L.gm_ffn_x1_plan(*args)
        assert e.value.code == L.EINVAL


# ------------------------------------------------------------------------------------------------ the knob
def test_knob_parsing(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    assert N.KeepNet(**DEFAULT_ARCH).flow_ffn_precision == 'x3'
    for v in ('x3', 'f16'):
        monkeypatch.setenv(KNOB, v)
        assert N.KeepNet(**DEFAULT_ARCH).flow_ffn_precision == v
    monkeypatch.setenv(KNOB, 'fp16')
    with pytest.raises(ValueError, match=KNOB):
        N.KeepNet(**DEFAULT_ARCH)
    monkeypatch.delenv(KNOB)
    net = N.KeepNet(**DEFAULT_ARCH)
    assert net.set_flow_ffn_precision('f16').flow_ffn_precision == 'f16' and net.set_flow_ffn_precision('x3').flow_ffn_precision == 'x3'
    for bad in ('bf16', 'fp32', '', None):
        with pytest.raises(ValueError, match=KNOB):
            net.set_flow_ffn_precision(bad)
    assert N.FLOW_FFN_PRECISIONS == ('x3', 'f16') and N.FLOW_PRECISIONS == ('x3', 'f16') and N.PRECISIONS == ('fp32', 'x3', 'bf16', 'f16')
    assert N.KNOB_OFF['flow_ffn_precision'] == 'x3' and N.FLOW_FFN_PRECISION_ENV == KNOB
    # independent of the flow knob
    monkeypatch.setenv('KEEP_AMD_FLOW_PRECISION', 'f16')
    other = N.KeepNet(**DEFAULT_ARCH)
    assert (other.flow_precision, other.flow_ffn_precision) == ('f16', 'x3')
    assert other.set_flow_ffn_precision('f16').flow_precision == 'f16' and other.set_flow_precision('x3').flow_ffn_precision == 'f16'


@pytest.mark.parametrize('base', ['fp32', 'bf16'])
def test_knob_needs_an_x3_grade_base(base, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    net = N.KeepNet(**DEFAULT_ARCH).set_precision(base).set_flow_ffn_precision('f16')
    with pytest.raises(ValueError, match=KNOB):
        net._activate_flow_ffn_precision()
    net.set_flow_ffn_precision('x3')._activate_flow_ffn_precision()      # the knob off: nothing to refuse
    assert net.o.ffn_x1 is False
    for ok in ('x3', 'f16'):
        net.set_precision(ok).set_flow_ffn_precision('f16')._activate_flow_ffn_precision()      # (no weights resident: no twin to build)
        assert net.o.ffn_x1 is True


def test_knob_travels_with_the_pool_config_and_the_twin_bytes(monkeypatch, synth_weights):
    for k in (KNOB, 'KEEP_AMD_FLOW_PRECISION', 'KEEP_AMD_UPSAMPLE_PRECISION'):
        monkeypatch.delenv(k, raising=False)
    net = N.KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth_weights, strict=True)
    assert net.pool_config()['flow_ffn_precision'] == 'x3' and net.o.ffn_x1 is False
    n = int(net._blob.size)
    pairs = net.flow_ffn_names()
    assert len(pairs) == 6 and all(a.endswith('.cross_attn_ffn.mlp.0.weight') and b.endswith('.cross_attn_ffn.mlp.2.weight') for a, b in pairs)
    shapes = [tuple(net._index[m][1]) for pair in pairs for m in pair]
    assert set(shapes) == {(1024, 256), (128, 1024)}
    ffn_bytes = sum(2 * a * b for a, b in shapes)      # one fp16 per weight
    assert ffn_bytes == 6 * 2 * (1024 * 256 + 128 * 1024)
    assert net.twin_bytes('x3') == 4 * n and net.twin_bytes('f16') == 6 * n and net.twin_bytes('bf16') == 2 * n      # the knob off: the pinned figures
    net.set_flow_precision('f16')
    assert net.twin_bytes('x3') == 6 * n and net.twin_bytes('f16') == 8 * n
    net.set_flow_precision('x3').set_flow_ffn_precision('f16')
    assert net.twin_bytes('x3') == 4 * n + ffn_bytes and net.twin_bytes('f16') == 6 * n + ffn_bytes and net.twin_bytes('bf16') == 2 * n
    assert set(net._twins('x3')) == {'x3', 'ffn'} and net._twins('x3')['ffn'] == (ffn_bytes, False)
    cfg = net.pool_config()
    assert cfg['flow_ffn_precision'] == 'f16' and cfg['flow_precision'] == 'x3'
    other = N.KeepNet(**DEFAULT_ARCH)
    other.apply_pool_config(cfg)
    assert other.flow_ffn_precision == 'f16' and other.precision == net.precision
    other.apply_pool_config({k: v for k, v in cfg.items() if k != 'flow_ffn_precision'})      # a root without the knob: the default
    assert other.flow_ffn_precision == 'x3'


# ------------------------------------------------------------------------------------------------ Ops.gm_ffn against a stubbed library
C_, HD = 128, 64


def _ops_with_blobs():
    """An x3 Ops over a CPU blob that holds W0 [HD, 2C] and W2 [C, HD] back to back, with a real x3 twin and per-tensor scales."""
    g = torch.Generator().manual_seed(11)
    n0, n2 = HD * 2 * C_, C_ * HD
    blob = torch.cat([0.08 * torch.randn(n0, generator=g), 0.05 * torch.randn(n2, generator=g)])
    index = {'w0': (0, (HD, 2 * C_)), 'w2': (n0, (C_, HD))}
    w = {'w0': blob[:n0].view(HD, 2 * C_), 'w2': blob[n0:].view(C_, HD)}
    bx3, table = ops.make_x3_blob(blob, index, w, ['w0', 'w2'])
    o = ops.Ops()
    o.set_precision(L.MMA_X3, blob, None, bx3, 1.0, x3_scales=table)
    return o, w['w0'], w['w2']


def _ffn_through_a_stub(monkeypatch, o, w0, w2, answer=None, Ms=(256, 300, 256)):
    """Ops.gm_ffn on CPU tensors for several token counts: the plan is a recorder that answers True, or raises ``answer``; the launch is a
    recorder.  Returns (plan queries, launches as (symbol, w0 twin pointer, w0 scale, w2 twin pointer, w2 scale, M, C, hidden, exact))."""
    plans, launches = [], []

    def plan(*args):
        plans.append(args)
        if answer is not None:
            raise answer
        return True

    def call(name, *a):
        launches.append((name, a[2].data_ptr(), a[3], a[4].data_ptr(), a[5], a[10], a[11], a[12], a[13]))
    monkeypatch.setattr(L, 'gm_ffn_x1_plan', plan)
    monkeypatch.setattr(L, 'call', call)
    g, b = torch.ones(C_), torch.zeros(C_)
    for M in Ms:
        out = o.gm_ffn(torch.zeros(M, C_), torch.zeros(M, C_), w0, w2, g, b, 1e-5)
        assert out.shape == (M, C_)
    return plans, launches


def test_rule_off_is_the_x3_symbol_with_the_x3_twins_and_no_plan_query(monkeypatch):
    o, w0, w2 = _ops_with_blobs()
    assert o.ffn_x1 is False
    plans, launches = _ffn_through_a_stub(monkeypatch, o, w0, w2)
    w2p, asc2 = o.ffn_w2_twin(w2)
    assert plans == [] and o._ffn_x1_route == {}
    assert launches == [('keep_gm_ffn_x3', o.x3_twin(w0).data_ptr(), o.x3_scale_of(w0), w2p.data_ptr(), asc2, M, C_, HD, 0) for M in (256, 300, 256)]
    assert not any(isinstance(k, tuple) and k[0] in ('ffn_w0_x1', 'ffn_w2_x1') for k in o._up2)      # and no hi-only twin was built


def test_rule_on_asks_once_per_key_and_launches_x1_with_the_hi_only_twins_and_the_x3_scales(monkeypatch):
    o, w0, w2 = _ops_with_blobs()
    o.ffn_x1 = True
    plans, launches = _ffn_through_a_stub(monkeypatch, o, w0, w2)
    (t0, a0), (t2, a2) = o.ffn_w0_x1_twin(w0), o.ffn_w2_x1_twin(w2)
    assert plans == [(C_, HD, 0, 0, 0)]                                       # one query for three calls of two token counts: M is no part of the key
    assert a0 == o.x3_scale_of(w0) and a2 == o.ffn_w2_twin(w2)[1]
    assert launches == [('keep_gm_ffn_x1', t0.data_ptr(), a0, t2.data_ptr(), a2, M, C_, HD, 0) for M in (256, 300, 256)]
    assert o._ffn_x1_route == {(C_, HD, 0, 0, 0): True}
    o.flags |= L.CONV_X3_EXACT_ACT                                            # the exact-erf flag travels
    _, launches = _ffn_through_a_stub(monkeypatch, o, w0, w2, Ms=(8,))
    assert launches[0][0] == 'keep_gm_ffn_x1' and launches[0][-1] == 1
    o.set_precision(L.MMA_X3, o.blob32, None, o.blobx3, 1.0, x3_scales=o._x3_table[1])      # a policy change forgets the routes, not the rule
    assert o._ffn_x1_route == {} and o.ffn_x1 is True


def test_eunsup_keeps_the_call_on_x3_cached_and_other_errors_propagate(monkeypatch):
    o, w0, w2 = _ops_with_blobs()
    o.ffn_x1 = True
    no = L.KeepHipError('keep_gm_ffn_x1_plan failed (code -2): keep_gm_ffn_x1_plan: the single-fp16 form is built for C = 128', code=L.EUNSUP)
    plans, launches = _ffn_through_a_stub(monkeypatch, o, w0, w2, answer=no)
    assert len(plans) == 1 and o._ffn_x1_route == {(C_, HD, 0, 0, 0): False}      # asked once, refused once, cached
    assert [l[0] for l in launches] == ['keep_gm_ffn_x3'] * 3 and launches[0][1] == o.x3_twin(w0).data_ptr()
    o2, w0b, w2b = _ops_with_blobs()
    o2.ffn_x1 = True
    bad = L.KeepHipError('keep_gm_ffn_x1_plan failed (code -1): keep_gm_ffn_x1_plan: bad args', code=L.EINVAL)
    plans, launches = [], []
    with pytest.raises(L.KeepHipError, match='code -1'):
        _ffn_through_a_stub(monkeypatch, o2, w0b, w2b, answer=bad)
    assert o2._ffn_x1_route == {}                                               # nothing cached


def test_against_the_built_library_the_workload_shape_is_admitted(monkeypatch):
    """The real keep_gm_ffn_x1_plan (host C) behind Ops.gm_ffn: admitted for the blob's aligned tensors; a misaligned activation view is
    the library's EUNSUP, so that call stays on x3."""
    o, w0, w2 = _ops_with_blobs()
    o.ffn_x1 = True
    launches = []
    monkeypatch.setattr(L, 'call', lambda name, *a: launches.append(name))
    g, b = torch.ones(C_), torch.zeros(C_)
    o.gm_ffn(torch.zeros(40, C_), torch.zeros(40, C_), w0, w2, g, b, 1e-5)
    off = torch.zeros(40 * C_ + 1)[1:].view(40, C_)      # 4 bytes off the allocation's alignment
    assert off.data_ptr() % 16 == 4
    o.gm_ffn(off, torch.zeros(40, C_), w0, w2, g, b, 1e-5)
    assert launches == ['keep_gm_ffn_x1', 'keep_gm_ffn_x3']
    assert sorted(o._ffn_x1_route.values()) == [False, True]


# ------------------------------------------------------------------------------------------------ the twin builders
def test_hi_only_twins_are_the_hi_halves_of_the_x3_twins_bit_for_bit():
    o, w0, w2 = _ops_with_blobs()
    (t0, a0), (t2, a2) = o.ffn_w0_x1_twin(w0), o.ffn_w2_x1_twin(w2)
    assert t0.dtype == t2.dtype == torch.int16 and t0.numel() == w0.numel() and t2.numel() == w2.numel()
    assert t0.data_ptr() % 16 == 0 and t2.data_ptr() % 16 == 0
    hi0 = o.x3_twin(w0).view(HD, 2 * C_ // 16, 2, 16)[:, :, 0, :].reshape(-1)      # [rows, Cin / 16, hi | lo, 16]
    assert torch.equal(t0, hi0) and a0 == o.x3_scale_of(w0)
    w2p, asc2 = o.ffn_w2_twin(w2)
    hi2 = w2p.view(C_, HD // 16, 2, 16)[:, :, 0, :].reshape(-1)
    assert torch.equal(t2, hi2) and a2 == asc2
    # and they are what their docstrings say: fp16(W * 2^e), W2 permuted
    assert torch.equal(t0.view(torch.float16), (w0 * (1.0 / a0)).to(torch.float16).view(-1))
    assert torch.equal(t2.view(torch.float16), (ops.ffn_w2_perm(w2) * (1.0 / a2)).to(torch.float16).view(-1))
    assert o.ffn_w0_x1_twin(w0)[0] is t0 and o.ffn_w2_x1_twin(w2)[0] is t2          # built once per weight tensor
