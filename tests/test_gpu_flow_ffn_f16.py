"""GPU suite (-m gpu): the opt-in single-fp16 form of GMFlow's fused feed-forward block (KEEP_AMD_FLOW_FFN_PRECISION=f16 /
KeepNet.set_flow_ffn_precision('f16'): every keep_gm_ffn_x3 launch of a GMFlow pass as keep_gm_ffn_x1) on an x3 base with and without flow 'f16'
-- flow quality on the reference golden beside 'bf16', the whole net with the reference's indices injected, batch invariance, the untouched
default and a knob set behind a replayed graph.  Every test builds its own networks."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import synth
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
from comfyui_keep_amd.engine.net import KeepNet

pytestmark = pytest.mark.gpu

# One GMFlow pass launches the fused FFN once per transformer layer: 6 (net.py:_gm_layer, the two images of a pair ride one launch).  The 12 of
# profiles/r06_x3_b48_kernel_stats.txt are the two GMFlow launch groups of a 48-clip step.
FFN_LAUNCHES_PER_PASS = 6

# Measured on the first green run (MI355X, 2026-10-20; DESIGN 4.7, profiles/f16_flow_ffn.txt).  The test allows twice the constant (reduction order of the
# statistics kernels from box to box) and demands strictly less than 'bf16' measured in the same run.  Not the 1e-3 parity tolerance: this
# mode is outside it.
#   max |flow - reference flow| in px on tests/golden/gmflow256.npz: (x3 + ffn f16, x3 + flow f16 + ffn f16)
# (same run, max / median px: x3 6.8474e-04 / 4.9393e-05, x3 + ffn f16 2.8458e-03 / 1.1822e-04, x3 + flow f16 1.7447e-01 / 6.9775e-03,
#  x3 + flow f16 + ffn f16 1.8761e-01 / 7.0171e-03, bf16 2.6723 / 6.4896e-02; flow scale 86.5 px)
FLOW_FFN_MAX_PX_MEASURED = {'x3+ffn': 2.8458e-03, 'x3+flow+ffn': 1.8761e-01}


def build(weights, precision, flow='x3', ffn='x3'):
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(weights, strict=True)
    return net.to('cuda').eval().set_precision(precision).set_flow_precision(flow).set_flow_ffn_precision(ffn)


class Spy:
    """Records every flat entry point that reaches the binding by name, and every keep_gm_ffn_x1_plan query."""

    def __init__(self, monkeypatch):
        self.calls, self.plan_queries = [], 0
        call, plan = L.call, L.gm_ffn_x1_plan

        def spy_call(name, *a):
            self.calls.append(name)
            return call(name, *a)

        def spy_plan(*a):
            self.plan_queries += 1
            return plan(*a)
        monkeypatch.setattr(L, 'call', spy_call)
        monkeypatch.setattr(L, 'gm_ffn_x1_plan', spy_plan)

    def ffn(self, n0=0):
        mine = self.calls[n0:]
        return mine.count('keep_gm_ffn_x3'), mine.count('keep_gm_ffn_x1')


def flow_of(net, a, dt):
    with torch.cuda.device(net.device):
        net._activate_precision()
        net.o.begin_forward(net.device)
        if net.of is not net.o:
            net.of.begin_forward(net.device)
        f = net._gmflow(a[dt:dt + 1].cuda(), a[0:1].cuda())
        torch.cuda.synchronize()
    return f.permute(0, 3, 1, 2).cpu().numpy()


def test_gmflow_alone_against_the_reference_golden_beside_bf16(synth_weights, monkeypatch):
    g = np.load(os.path.join(GOLDEN, 'gmflow256.npz'))
    dt = int(g['dt'])
    a = synth.synth_clip(T=dt + 1, B=1, size=256, seed=int(g['clip_seed']))[0]
    ref = g['flow']
    spy = Spy(monkeypatch)
    rep, flows = {}, {}
    settings = (('x3', ('x3', 'x3', 'x3')), ('x3+ffn', ('x3', 'x3', 'f16')), ('x3+flow', ('x3', 'f16', 'x3')), ('x3+flow+ffn', ('x3', 'f16', 'f16')),
                ('bf16', ('bf16', 'x3', 'x3')))
    for pol, (base, flow, ffn) in settings:
        net = build(synth_weights, base, flow, ffn)
        n0, q0 = len(spy.calls), spy.plan_queries
        f = flows[pol] = flow_of(net, a, dt)
        assert np.isfinite(f).all(), pol
        err = np.sqrt(((f - ref) ** 2).sum(1))
        rep[pol] = (float(np.abs(f - ref).max()), float(np.median(err)))
        if ffn == 'f16':      # every FFN launch of the pass is the x1 symbol, none the x3 one; one plan query for the one shape key
            assert spy.ffn(n0) == (0, FFN_LAUNCHES_PER_PASS) and spy.plan_queries == q0 + 1 and net.o.ffn_x1 is True, (pol, spy.ffn(n0))
        elif base == 'x3':    # the reverse, and the library is never asked
            assert spy.ffn(n0) == (FFN_LAUNCHES_PER_PASS, 0) and spy.plan_queries == q0 and net.o.ffn_x1 is False, (pol, spy.ffn(n0))
        del net
    print('[flow-ffn-f16] gmflow256 flow error in px (max, median): ' + ', '.join(f'{k} {v}' for k, v in rep.items()) +
          f'; scale {float(np.abs(ref).max()):.3g} px')
    assert rep['x3'][0] <= 2e-3                                       # x3 has not moved (5.4e-4 px, tests/test_gpu_net.py)
    for pol, off in (('x3+ffn', 'x3'), ('x3+flow+ffn', 'x3+flow')):
        assert not np.array_equal(flows[pol], flows[off]), pol        # differs from the same setting without the knob
        assert rep[pol][0] < rep['bf16'][0] and rep[pol][1] < rep['bf16'][1], rep
        assert FLOW_FFN_MAX_PX_MEASURED[pol] is not None, f'FLOW_FFN_MAX_PX_MEASURED not recorded yet; measured {rep}'
        assert rep[pol][0] <= 2.0 * FLOW_FFN_MAX_PX_MEASURED[pol], rep


def test_whole_net_with_injected_indices_equals_the_base_bit_for_bit(synth_weights):
    """With the reference's indices injected the flows reach the pixels only through the code indices -- which are forced -- so the
    knob leaves the base's pixels where they were, bit for bit, and nothing falls back."""
    g = np.load(os.path.join(GOLDEN, 'keep_forward_T3.npz'))
    x = synth.synth_clip(T=3, B=1, seed=1234).cuda()
    forced = torch.from_numpy(g['indices'].astype(np.int32)).view(1, 3, -1)
    for base, flow in (('x3', 'x3'), ('x3', 'f16')):
        outs = {}
        for ffn in ('x3', 'f16'):
            net = build(synth_weights, base, flow, ffn)
            outs[ffn] = net(x, force_indices=forced)
            assert torch.isfinite(outs[ffn]).all() and net.x3_fallbacks == 0, (base, flow, ffn)
            assert net.o.ffn_x1 is (ffn == 'f16')
            del net
        assert torch.equal(outs['f16'], outs['x3']), (base, flow)


def test_batch_of_two_clips_equals_one_by_one(synth_weights):
    net = build(synth_weights, 'x3', 'x3', 'f16')
    x = torch.cat([synth.synth_clip(T=3, B=1, seed=1234), synth.synth_clip(T=3, B=1, seed=77, phase=1.0)], 0).cuda()
    both, aux = net(x, return_aux=True)
    for b in range(2):
        one, aux1 = net(x[b:b + 1], return_aux=True)
        assert torch.equal(aux1['indices'][0], aux['indices'][b])
        assert torch.equal(one[0], both[b])
    with torch.cuda.device(net.device):      # and the flow field itself, pair by pair
        net._activate_precision()
        f2 = net._gmflow_clip(x)
        f1 = torch.cat([net._gmflow_clip(x[b:b + 1]) for b in range(2)], 0)
        torch.cuda.synchronize()
    assert torch.equal(f1, f2) and net.o.ffn_x1 is True and list(net.o._ffn_x1_route.values()) == [True]


def test_knob_unset_is_the_x3_network_launch_for_launch(synth_weights, monkeypatch):
    """With the knob unset the T = 3 forward is the x3 forward: no plan query, no launch of the x1 symbol, no hi-only FFN twin, and the result
    equals -- bit for bit, same launch census, same flat entry points in the same order -- a net that ran under the knob and was switched back."""
    monkeypatch.delenv('KEEP_AMD_FLOW_FFN_PRECISION', raising=False)
    x = synth.synth_clip(T=3, B=1, seed=1234).cuda()
    spy = Spy(monkeypatch)
    plain = KeepNet(**DEFAULT_ARCH)
    plain.load_state_dict(synth_weights, strict=True)
    plain.to('cuda').eval()
    assert plain.precision == 'x3' and plain.flow_ffn_precision == 'x3'
    plain.graph_mode = '0'
    plain.o.census = c_plain = {}
    out = plain(x)
    calls_plain = list(spy.calls)
    n_ffn = spy.ffn()[0]
    assert spy.plan_queries == 0 and spy.ffn() == (n_ffn, 0) and n_ffn >= FFN_LAUNCHES_PER_PASS and n_ffn % FFN_LAUNCHES_PER_PASS == 0 and plain.o.ffn_x1 is False
    assert not any(isinstance(k, tuple) and k[0] in ('ffn_w0_x1', 'ffn_w2_x1') for k in plain.o._up2)
    other = build(synth_weights, 'x3', 'x3', 'f16')
    other.graph_mode = '0'
    n0 = len(spy.calls)
    moved = other(x)
    # (the pixels need not move: un-forced, the flows reach them only through code indices that may all stay -- the flow itself is judged above)
    assert spy.plan_queries == 1 and spy.ffn(n0) == (0, n_ffn) and torch.isfinite(moved).all()
    other.set_flow_ffn_precision('x3')
    other.o.census = c_other = {}
    n0 = len(spy.calls)
    back = other(x)
    assert spy.plan_queries == 1 and other.o.ffn_x1 is False
    assert spy.calls[n0:] == calls_plain and c_other == c_plain and torch.equal(back, out)


def test_knob_set_behind_a_replayed_graph_takes_effect_on_the_next_call(synth_weights, monkeypatch):
    """B = 1 with hipGraph replay: the knob is part of the graph key, so toggling it between two forwards of one shape never replays the other
    setting's graph -- each setting has the bits of an eager net that had it from the start."""
    x = synth.synth_clip(T=2, B=1, seed=1234).cuda()
    net = build(synth_weights, 'x3')
    net.graph_mode = '1'
    first = net(x).clone()
    again = net(x).clone()                      # a replay
    assert len(net._graphs) == 1 and torch.equal(first, again)
    net.set_flow_ffn_precision('f16')
    spy = Spy(monkeypatch)
    moved = net(x).clone()                      # eager pass + capture under the knob
    assert spy.ffn()[0] == 0 and spy.ffn()[1] >= FFN_LAUNCHES_PER_PASS      # the other kernel sequence ran and was captured, not the x3 graph replayed
    k_off, k_on = list(net._graphs)
    assert len(net._graphs) == 2 and [a for a, b in zip(k_off, k_on) if a != b] == ['x3'] and [b for a, b in zip(k_off, k_on) if a != b] == ['f16']
    eager = build(synth_weights, 'x3', 'x3', 'f16')
    eager.graph_mode = '0'
    assert torch.equal(eager(x), moved)
    n0 = len(spy.calls)
    assert torch.equal(net(x), moved)           # the replay of the second graph
    net.set_flow_ffn_precision('x3')
    assert torch.equal(net(x), first) and len(net._graphs) == 2      # and back: the first graph, not the second
    assert 'keep_gm_ffn_x1' not in spy.calls[n0:] and 'keep_gm_ffn_x3' not in spy.calls[n0:]      # both were replays
