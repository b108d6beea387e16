"""GPU suite (-m gpu): GMFlow's opt-in single-fp16 precision (KEEP_AMD_FLOW_PRECISION=f16 / KeepNet.set_flow_precision('f16'): the CNN backbone,
the swin blocks and the q / k projections on KEEP_MMA_X1 where the library admits it; correlation, propagation, the fused FFN and the
upsampler on x3) -- flow quality on the reference golden beside 'bf16', pixel quality of the whole net, batch invariance, and the untouched
default.  Every test builds its own networks (the session's `gpu_net` fixture keeps its two policies)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops, synth
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
from comfyui_keep_amd.engine.net import KeepNet

pytestmark = pytest.mark.gpu

# Measured on the first green run (MI355X, 2026-10-18; DESIGN 4.5, profiles/f16_flow_precision.txt).  The tests allow twice the constant
# (reduction order of the statistics kernels from box to box) and demand strictly less than 'bf16' measured in the same run.  Not the 1e-3
# parity tolerance: this mode is outside it.
#   max |flow - reference flow| in px on tests/golden/gmflow256.npz under x3 + flow f16
FLOW_F16_MAX_PX_MEASURED = 1.7447e-01      # (same run: median 6.9775e-03 px; bf16 2.6723 / 6.4896e-02 px, x3 6.8474e-04 / 4.9393e-05 px; flow scale 86.5 px)
#   max |pixel - reference| on the T = 3 golden's 32 x 32 digest with the reference's indices injected: (x3 + flow f16, f16 + flow f16)
PIXEL_ERR_MEASURED = {'x3+flow': 1.3903e-05, 'f16+flow': 3.5299e-03}      # (same run: bf16 4.0754e-02, x3 1.3903e-05; output scale 1.01)


def build(weights, precision, flow='x3'):
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(weights, strict=True)
    return net.to('cuda').eval().set_precision(precision).set_flow_precision(flow)


def digest(frames):
    T, C, H, Wd = frames.shape
    return frames[:, :, 7::H // 32, 5::Wd // 32][:, :, :32, :32]


class Spy:
    """Records what reaches the binding: every keep_attention launch as (mma, flags, Dv), every X1 plan query of either entry point."""

    def __init__(self, monkeypatch):
        self.launches, self.attn_queries, self.conv_x1_queries = [], 0, 0
        attention, attn_plan, conv_plan = L.attention, L.attention_x1_plan, L.conv2d_plan

        def spy_attention(**kw):
            self.launches.append((kw['mma'], kw['flags'], kw['Dv']))
            return attention(**kw)

        def spy_attn_plan(**kw):
            self.attn_queries += 1
            return attn_plan(**kw)

        def spy_conv_plan(a):
            self.conv_x1_queries += int(a.mma == L.MMA_X1)
            return conv_plan(a)
        monkeypatch.setattr(L, 'attention', spy_attention)
        monkeypatch.setattr(L, 'attention_x1_plan', spy_attn_plan)
        monkeypatch.setattr(L, 'conv2d_plan', spy_conv_plan)


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
    rep, census = {}, {}
    for pol, net in (('x3', build(synth_weights, 'x3')), ('x3+flow', build(synth_weights, 'x3', 'f16')), ('bf16', build(synth_weights, 'bf16'))):
        net.o.census = census[pol] = {}
        n0 = len(spy.launches)
        flow = flow_of(net, a, dt)
        assert np.isfinite(flow).all(), pol
        err = np.sqrt(((flow - ref) ** 2).sum(1))
        rep[pol] = (float(np.abs(flow - ref).max()), float(np.median(err)))
        if pol == 'x3':
            assert spy.attn_queries == 0 and spy.conv_x1_queries == 0 and all(m == L.MMA_X3 for m, _, _ in spy.launches[n0:])
        if pol == 'x3+flow':
            mine = spy.launches[n0:]
            # the 12 window attentions run the flagged form; the correlation and the propagation (Dv = 2) stay x3, never asked about
            assert [m for m, _, dv in mine if dv == 128] == [L.MMA_X1] * 12 and all(f & L.ATTN_X1 for m, f, dv in mine if dv == 128)
            assert [m for m, _, dv in mine if dv == 2] == [L.MMA_X3] * 2 and not any(f & L.ATTN_X1 for m, f, dv in mine if dv == 2)
            assert net.of is not net.o and net.of.attn_x1 and not net.o.attn_x1 and net.o.blobx1 is None
    print(f'[flow-f16] gmflow256 flow error in px (max, median): x3 {rep["x3"]}, x3 + flow f16 {rep["x3+flow"]}, bf16 {rep["bf16"]}; '
          f'scale {float(np.abs(ref).max()):.3g} px')
    print('[flow-f16] census x3     :', sorted(census['x3'].items()), '\n[flow-f16] census x3+flow:', sorted(census['x3+flow'].items()))
    assert rep['x3'][0] <= 2e-3                                       # x3 has not moved (5.4e-4 px, tests/test_gpu_net.py)
    assert set(census['x3+flow']) - set(census['x3']), 'no single-fp16 convolution was launched'      # (X1 plans carry their own kernel names)
    assert rep['x3+flow'][0] > rep['x3'][0]                            # really single-fp16 kernels
    assert rep['x3+flow'][0] < rep['bf16'][0] and rep['x3+flow'][1] < rep['bf16'][1], rep
    assert FLOW_F16_MAX_PX_MEASURED is not None, f'FLOW_F16_MAX_PX_MEASURED not recorded yet; measured {rep}'
    assert rep['x3+flow'][0] <= 2.0 * FLOW_F16_MAX_PX_MEASURED, rep


def test_whole_net_against_the_reference_golden_beside_bf16(synth_weights):
    g = np.load(os.path.join(GOLDEN, 'keep_forward_T3.npz'))
    x = synth.synth_clip(T=3, B=1, seed=1234).cuda()
    forced = torch.from_numpy(g['indices'].astype(np.int32)).view(1, 3, -1)
    err, outs = {}, {}
    for pol, (base, flow) in (('x3+flow', ('x3', 'f16')), ('f16+flow', ('f16', 'f16')), ('bf16', ('bf16', 'x3')), ('x3', ('x3', 'x3'))):
        net = build(synth_weights, base, flow)
        out = net(x, force_indices=forced)
        assert torch.isfinite(out).all() and net.x3_fallbacks == 0, pol
        err[pol] = float(np.abs(digest(out[0].cpu()).numpy() - g['out_grid']).max())
        outs[pol] = out.cpu()
        del net, out
    print('[flow-f16] max-abs pixel error, reference indices injected (T = 3): ' + ', '.join(f'{k} {v:.4e}' for k, v in err.items()) +
          f'; output scale {float(np.abs(g["out_grid"]).max()):.3g}')
    # Measured, and stated rather than hidden: with the reference's indices injected the flows reach the pixels only through the code
    # indices -- which are forced -- so on this golden flow 'f16' leaves the base policy's pixels bit for bit where they were.  The un-forced
    # forward does move (test_knob_unset_is_the_x3_network_launch_for_launch); its yardstick is the flow error above.
    assert torch.equal(outs['x3+flow'], outs['x3'])
    for pol in ('x3+flow', 'f16+flow'):
        assert err[pol] < err['bf16'], err
        assert PIXEL_ERR_MEASURED[pol] is not None, f'PIXEL_ERR_MEASURED not recorded yet; measured {err}'
        assert err[pol] <= 2.0 * PIXEL_ERR_MEASURED[pol], err


def test_flow_f16_batch_of_two_clips_equals_one_by_one(synth_weights):
    net = build(synth_weights, 'x3', 'f16')
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
    assert torch.equal(f1, f2)


def test_knob_unset_is_the_x3_network_launch_for_launch(synth_weights, monkeypatch):
    """With the knob unset the T = 3 forward is the x3 forward: ``of`` is ``o``, no launch carries KEEP_MMA_X1 / KEEP_ATTN_X1, no X1 plan is
    ever queried, and the result equals -- bit for bit, same launch census -- a net that ran under flow 'f16' and was switched back."""
    monkeypatch.delenv('KEEP_AMD_FLOW_PRECISION', raising=False)
    x = synth.synth_clip(T=3, B=1, seed=1234).cuda()
    spy = Spy(monkeypatch)
    plain = KeepNet(**DEFAULT_ARCH)
    plain.load_state_dict(synth_weights, strict=True)
    plain.to('cuda').eval()
    assert plain.precision == 'x3' and plain.flow_precision == 'x3'
    plain.graph_mode = '0'
    plain.o.census = c_plain = {}
    out = plain(x)
    assert plain.of is plain.o and plain._of is None and plain._dev_blobx1f is None
    assert spy.attn_queries == 0 and spy.conv_x1_queries == 0 and spy.launches
    assert all(m != L.MMA_X1 and not (f & L.ATTN_X1) for m, f, _ in spy.launches)
    other = build(synth_weights, 'x3', 'f16')
    other.graph_mode = '0'
    moved = other(x)
    assert spy.attn_queries > 0 and not torch.equal(moved, out)
    n0, q0 = len(spy.launches), (spy.attn_queries, spy.conv_x1_queries)
    other.set_flow_precision('x3')
    other.o.census = c_other = {}
    back = other(x)
    assert other.of is other.o and (spy.attn_queries, spy.conv_x1_queries) == q0
    assert all(m != L.MMA_X1 and not (f & L.ATTN_X1) for m, f, _ in spy.launches[n0:])
    assert c_other == c_plain and torch.equal(back, out)
