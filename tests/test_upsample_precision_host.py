"""CPU: the host side of the generator's opt-in single-fp16 Upsample convolutions (KEEP_AMD_UPSAMPLE_PRECISION=f16) -- the third admitting
bit KEEP_CONV_X1_UP2 in header, binding and keep_conv2d_plan (host C: what the built library admits and what it refuses, with its reasons),
the KeepNet knob, and the routing rule of Ops.conv's up2 branch against a stubbed library."""
import os
import re

import pytest
import torch

from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import net as N
from comfyui_keep_amd.engine import ops
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = 'KEEP_AMD_UPSAMPLE_PRECISION'
X3_PHASES = 'conv3x3_halo_x3_kernel<32, x2 phases>'


def test_bit_in_header_and_binding():
    header = open(os.path.join(ROOT, 'include', 'keep_hip.h')).read()
    assert L.CONV_X1_UP2 == 1 << 16 and L.ABI_VERSION == 23
    assert re.search(r'#define KEEP_CONV_X1_UP2 \(1u << 16\)', header)
    assert int(re.search(r'#define KEEP_ABI_VERSION (\d+)', header).group(1)) == 23
    assert ops.X1_UP2_KERNEL != X3_PHASES and ops.X1_UP2_KERNEL != ops.X3_STREAM_KERNEL


def _plan(**kw):
    """The issue's call: N = 2, a 32 x 128 source map, 128 -> 128 channels, the hi-only phase twin, KEEP_MMA_X1 with the bit."""
    buf = torch.zeros(64, dtype=torch.float32)
    ptr = buf.data_ptr() // 16 * 16 + 16
    base = dict(N=2, H=32, W=128, Cin=128, Cout=128, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=64, Wo=256, in_ld=128, out_ld=128,
                mma=L.MMA_X1, upsample=L.UPSAMPLE_X2_PHASES, inp=ptr, out=ptr, weight=ptr, weight_x3=ptr, x3_acc_scale=1.0,
                flags=L.CONV_X1_UP2, pad_mode=L.PAD_ZERO)
    base.update(kw)
    L.load(check_device=False)
    return L.conv2d_plan(L.conv_args(**base)), ptr


def test_plan_with_the_bit():
    pl, _ = _plan()
    x3, _ = _plan(mma=L.MMA_X3, flags=0)
    assert pl.kernel.decode() == ops.X1_UP2_KERNEL and x3.kernel.decode() == X3_PHASES
    assert pl.split_k == 1 and pl.workspace_bytes == 0
    assert (pl.stats_P, pl.stats_rows, pl.out_amax_ok) == (x3.stats_P, x3.stats_rows, x3.out_amax_ok) == (64 * 256 // 256, 256, 1)
    # every other policy ignores the bit
    assert _plan(mma=L.MMA_X3)[0].kernel.decode() == X3_PHASES
    # the plan follows the per-image geometry, never N
    seen = set()
    for n in (1, 2, 16):
        p_, _ = _plan(N=n)
        seen.add((p_.kernel.decode(), p_.split_k, p_.stats_rows, p_.stats_P, p_.out_amax_ok, p_.path))
    assert len(seen) == 1, seen
    # strided slices, a residual in place and a bias stay admitted
    _, ptr = _plan()
    assert _plan(in_ld=160, out_ld=192, residual=ptr, res_ld=192, bias=ptr)[0].kernel.decode() == ops.X1_UP2_KERNEL


def test_without_the_bit_x1_phases_stay_refused():
    for flags in (0, L.CONV_X1_GEMM | L.CONV_X1_HALO16):
        with pytest.raises(L.KeepHipError, match='keep_conv2d'):
            _plan(flags=flags)


_PTR = 0x10000


@pytest.mark.parametrize('what,over,text', [
    ('depth', dict(Cin=48, in_ld=48), r'Cin % 32'),
    ('affine prologue', dict(pro_scale=_PTR, pro_shift=_PTR), 'prologue'),
    ('prologue activation', dict(pro_act=L.PRO_SWISH), 'prologue'),
    ('epilogue activation', dict(epi_act=L.ACT_RELU), 'activation'),
    ('aux', dict(aux=_PTR, residual=_PTR, res_ld=128), 'aux'),
    ('in2', dict(in2=_PTR, in2_cin1=64), 'in2'),
    ('split-K', dict(split_k=2), 'split'),
    ('reflection padding', dict(pad_mode=L.PAD_REFLECT), 'KEEP_PAD_REFLECT'),
    ('a map and Cout the phase form refuses', dict(H=12, W=48, Ho=24, Wo=96, Cout=96, out_ld=96), 'phase form'),
    ('no twin', dict(weight_x3=None), 'twin'),
    ('the stage-barrier form', dict(flags=L.CONV_X1_UP2 | L.CONV_NO_STREAM), 'phase form'),
])
def test_with_the_bit_everything_else_is_refused_with_its_reason(what, over, text):
    with pytest.raises(L.KeepHipError) as e:
        _plan(**over)
    msg = str(e.value)
    # (in2 is refused before the planner: "a KEEP_MMA_X3 feature")
    assert '(code -2)' in msg and ('KEEP_MMA_X1' in msg or what == 'in2') and re.search(text, msg), (what, msg)


# ------------------------------------------------------------------------------------------------ the knob
def test_knob_parsing(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    assert N.KeepNet(**DEFAULT_ARCH).upsample_precision == 'x3'
    for v in ('x3', 'f16'):
        monkeypatch.setenv(KNOB, v)
        assert N.KeepNet(**DEFAULT_ARCH).upsample_precision == v
    monkeypatch.setenv(KNOB, 'fp16')
    with pytest.raises(ValueError, match=KNOB):
        N.KeepNet(**DEFAULT_ARCH)
    monkeypatch.delenv(KNOB)
    net = N.KeepNet(**DEFAULT_ARCH)
    assert net.set_upsample_precision('f16').upsample_precision == 'f16' and net.set_upsample_precision('x3').upsample_precision == 'x3'
    for bad in ('bf16', 'fp32', '', None):
        with pytest.raises(ValueError, match=KNOB):
            net.set_upsample_precision(bad)
    assert N.UPSAMPLE_PRECISIONS == ('x3', 'f16') and N.PRECISIONS == ('fp32', 'x3', 'bf16', 'f16')      # the base tuple is untouched


@pytest.mark.parametrize('base', ['fp32', 'bf16'])
def test_knob_needs_an_x3_grade_base(base, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    net = N.KeepNet(**DEFAULT_ARCH).set_precision(base).set_upsample_precision('f16')
    with pytest.raises(ValueError, match=KNOB):
        net._activate_upsample_precision()
    net.set_upsample_precision('x3')._activate_upsample_precision()      # the knob off: nothing to refuse
    assert net.o.up2_x1 is False


def test_knob_travels_with_the_pool_config_and_the_twin_bytes(monkeypatch, synth_weights):
    monkeypatch.delenv(KNOB, raising=False)
    net = N.KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth_weights, strict=True)
    assert net.pool_config()['upsample_precision'] == 'x3' and net.o.up2_x1 is False
    n = int(net._blob.size)
    from comfyui_keep_amd.engine.arch import generator_blocks
    all_ups = [f'generator.blocks.{i}.conv.weight' for i, (kind, _, _) in enumerate(generator_blocks(net.cfg)) if kind == 'up']
    # the 32^2, 64^2, 128^2 and 256^2 sources get a hi-only phase twin; the 16^2 -> 32^2 Upsample, which no phase form takes, gets none
    assert net.up2_x1_names() == all_ups[1:] and len(all_ups) == 5
    ups = [net._index[name][1] for name in net.up2_x1_names()]
    up_bytes = sum(4 * 2 * s[0] * s[1] * s[2] * s[3] for s in ups)      # four phase kernels of 2 bytes per weight
    assert up_bytes > 0
    assert net.twin_bytes('x3') == 4 * n and net.twin_bytes('f16') == 6 * n
    net.set_upsample_precision('f16')
    assert net.twin_bytes('x3') == 4 * n + up_bytes and net.twin_bytes('f16') == 6 * n + up_bytes and net.twin_bytes('bf16') == 2 * n
    cfg = net.pool_config()
    assert cfg['upsample_precision'] == 'f16'
    other = N.KeepNet(**DEFAULT_ARCH)
    other.apply_pool_config(cfg)
    assert other.upsample_precision == 'f16' and other.precision == net.precision
    other.apply_pool_config({k: v for k, v in cfg.items() if k != 'upsample_precision'})      # a root without the knob: the default
    assert other.upsample_precision == 'x3'


# ------------------------------------------------------------------------------------------------ Ops.conv against a stubbed library
_REAL_PLAN = L.conv2d_plan


def _conv_through_a_stub(monkeypatch, o, w, refuse=False, broken=False, N_=2):
    """Ops.conv(upsample=True) on CPU tensors: keep_conv2d_plan is the built library's (host C) behind a recorder -- or a stub that answers
    KEEP_EUNSUP / an error to X1 -- and the launch and the range probe are recorders.  Returns (plan queries, launches) as
    (mma, flags, weight_x3 pointer, x3_acc_scale)."""
    plans, launches = [], []

    def plan(a):
        plans.append((a.mma, a.flags, a.weight_x3, a.x3_acc_scale))
        if a.mma == L.MMA_X1 and refuse:
            raise L.KeepHipError('keep_conv2d_plan failed (code -2): keep_conv2d: KEEP_MMA_X1 (with KEEP_CONV_X1_UP2) has no kernel for this call', code=L.EUNSUP)
        if a.mma == L.MMA_X1 and broken:
            raise L.KeepHipError('keep_conv2d_plan failed (code -1): keep_conv2d: non-positive dimension', code=L.EINVAL)
        return _REAL_PLAN(a)

    monkeypatch.setattr(ops, '_PLAN_CACHE', {})
    monkeypatch.setattr(L, 'conv2d_plan', plan)
    monkeypatch.setattr(L, 'conv2d_launch', lambda a: launches.append((a.mma, a.flags, a.weight_x3, a.x3_acc_scale, a.upsample)))
    monkeypatch.setattr(L, 'call', lambda name, *args: None)
    x = torch.zeros(N_, 8, 32, w.shape[-1])
    for _ in range(3):
        o.conv(x, w, None, upsample=True)
    return plans, launches


def _ops_with_blobs(cin=32, cout=64):
    g = torch.Generator().manual_seed(5)
    blob = torch.randn(cout * 9 * cin, generator=g)
    o = ops.Ops()
    o.set_precision(L.MMA_X3, blob, None, torch.zeros(2 * blob.numel(), dtype=torch.int16), 1.0)
    return o, blob.view(cout, 3, 3, cin)


def test_knob_off_issues_no_x1_plan_query(monkeypatch):
    o, w = _ops_with_blobs()
    assert o.up2_x1 is False
    plans, launches = _conv_through_a_stub(monkeypatch, o, w)
    wx3 = o.up2_twin(w)[0].data_ptr()
    assert plans == [(L.MMA_X3, 0, wx3, plans[0][3])], plans                  # one base query per key, nothing under X1
    assert launches == [(L.MMA_X3, 0, wx3, plans[0][3], L.UPSAMPLE_X2_PHASES)] * 3
    assert o._up2_x1_route == {} and not any(isinstance(k, tuple) and k[0] == 'up2_x1' for k in o._up2)      # and no twin was built


def test_knob_on_queries_x1_with_the_phase_twin_and_the_bit(monkeypatch):
    o, w = _ops_with_blobs()
    o.up2_x1 = True
    plans, launches = _conv_through_a_stub(monkeypatch, o, w)
    tw, sc = o.up2_x1_twin(w)
    w4 = ops.up2_phase_weights(w)
    assert tw.dtype == torch.int16 and tw.numel() == 4 * w.numel() and tw.data_ptr() % 16 == 0
    assert sc == o.up2_twin(w)[1]                                             # the x3 phase twin's power of two
    assert torch.equal(tw.view(torch.float16).float(), (w4 * (1.0 / sc)).to(torch.float16).float().view(-1))
    assert len(plans) == 2 and plans[0][0] == L.MMA_X3 and plans[0][1] == 0
    assert plans[1] == (L.MMA_X1, L.CONV_X1_UP2, tw.data_ptr(), pytest.approx(sc)), plans      # one X1 query per plan key
    assert launches == [(L.MMA_X1, L.CONV_X1_UP2, tw.data_ptr(), pytest.approx(sc), L.UPSAMPLE_X2_PHASES)] * 3
    # the batch is no part of the route's key; a policy change forgets the routes
    assert len(o._up2_x1_route) == 1 and next(iter(o._up2_x1_route.values())).kernel == ops.X1_UP2_KERNEL
    o.set_precision(L.MMA_X3, o.blob32, None, o.blobx3, 1.0)
    assert o._up2_x1_route == {} and o.up2_x1 is True


def test_eunsup_keeps_the_call_on_x3_and_errors_propagate(monkeypatch):
    o, w = _ops_with_blobs()
    o.up2_x1 = True
    plans, launches = _conv_through_a_stub(monkeypatch, o, w, refuse=True)
    wx3 = o.up2_twin(w)[0].data_ptr()
    assert [p[0] for p in plans] == [L.MMA_X3, L.MMA_X1]                        # asked once, refused once
    assert [(m, f, p_) for m, f, p_, _, _ in launches] == [(L.MMA_X3, 0, wx3)] * 3
    o2, w2 = _ops_with_blobs()
    o2.up2_x1 = True
    with pytest.raises(L.KeepHipError, match='code -1'):
        _conv_through_a_stub(monkeypatch, o2, w2, broken=True)
    # a depth that is no multiple of 32 has no hi-only phase twin: no twin is built in the launch path and the library is not asked
    o3, w3 = _ops_with_blobs(cin=48)
    o3.up2_x1 = True
    plans, launches = _conv_through_a_stub(monkeypatch, o3, w3)
    assert [p[0] for p in plans] == [L.MMA_X3] and {m for m, *_ in launches} == {L.MMA_X3}
    assert not any(isinstance(k, tuple) and k[0] == 'up2_x1' for k in o3._up2)
