"""GPU suite (-m gpu): the generator's opt-in single-fp16 Upsample convolutions (KEEP_AMD_UPSAMPLE_PRECISION=f16 /
KeepNet.set_upsample_precision('f16'): the x2-phase Upsample convolutions on KEEP_MMA_X1 with KEEP_CONV_X1_UP2) on an 'x3' and on an 'f16'
base -- the launch census, quality against the reference golden between x3 and bf16, batch invariance, the fp16-range fallback, the untouched
default and a knob set behind a replayed graph.  Every test builds its own networks."""
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

X3_PHASES = 'conv3x3_halo_x3_kernel<32, x2 phases>'
F16_ERR_PARENT = 3.53e-3      # tests/test_gpu_net_f16.py: F16_ERR_MEASURED, precision 'f16' alone on the same golden


def build(weights, precision, upsample='x3'):
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(weights, strict=True)
    return net.to('cuda').eval().set_precision(precision).set_upsample_precision(upsample)


def digest(frames):
    T, C, H, Wd = frames.shape
    return frames[:, :, 7::H // 32, 5::Wd // 32][:, :, :32, :32]


@pytest.mark.parametrize('base', ['x3', 'f16'])
def test_exactly_the_phase_form_upsample_launches_move(base, synth_weights):
    """The launch census of one T = 2 forward, read through keep_conv2d_plan's kernel names: with the knob every x2-phase Upsample launch
    of the base (32^2, 64^2, 128^2 and 256^2 sources) runs under the new kernel string, and every other family is the base's, count for
    count -- the 16^2 -> 32^2 Upsample, which no phase form takes, included."""
    x = synth.synth_clip(T=2, B=1, seed=1234).cuda()
    census = {}
    for knob in ('x3', 'f16'):
        net = build(synth_weights, base, knob)
        net.graph_mode = '0'
        net.o.census = census[knob] = {}
        try:
            out = net(x)
        finally:
            net.o.census = None
        assert torch.isfinite(out).all() and net.x3_fallbacks == 0
        assert net.o.up2_x1 is (knob == 'f16') and net.o.mma == L.MMA_X3
    c0, c1 = census['x3'], census['f16']
    print(f'[up-f16-census] base {base}:', sorted(c0.items()), f'\n[up-f16-census] {base} + knob:', sorted(c1.items()))
    assert ops.X1_UP2_KERNEL not in c0 and c0[X3_PHASES] == 2 * 4                  # four phase-form Upsample convolutions per frame
    assert c1.get(X3_PHASES, 0) == 0 and c1[ops.X1_UP2_KERNEL] == c0[X3_PHASES]
    assert {k: n for k, n in c1.items() if k != ops.X1_UP2_KERNEL} == {k: n for k, n in c0.items() if k != X3_PHASES}


def test_golden_between_x3_and_bf16(synth_weights):
    """T = 3 golden with the reference's indices injected, four nets in one run: the knob's error on either base lies strictly above x3's
    (really single fp16) and strictly below bf16's (the labelled speed mode it must beat); no cap beyond that.  Printed: the ratio of
    f16 + knob to the figure 'f16' alone recorded on this golden (profiles/f16_upsample_precision.txt)."""
    g = np.load(os.path.join(GOLDEN, 'keep_forward_T3.npz'))
    x = synth.synth_clip(T=3, B=1, seed=1234).cuda()
    forced = torch.from_numpy(g['indices'].astype(np.int32)).view(1, 3, -1)
    err = {}
    for name, pol, knob in (('x3', 'x3', 'x3'), ('x3+up', 'x3', 'f16'), ('bf16', 'bf16', 'x3'), ('f16+up', 'f16', 'f16')):
        net = build(synth_weights, pol, knob)
        out = net(x, force_indices=forced)
        assert torch.isfinite(out).all() and net.x3_fallbacks == 0
        err[name] = float(np.abs(digest(out[0].cpu()).numpy() - g['out_grid']).max())
    print(f'[up-f16-golden] max-abs pixel error, reference indices injected (T = 3): x3 {err["x3"]:.4e}, x3 + knob {err["x3+up"]:.4e}, '
          f'f16 + knob {err["f16+up"]:.4e}, bf16 {err["bf16"]:.4e}; f16 + knob / f16 alone as recorded ({F16_ERR_PARENT:.2e}) = '
          f'{err["f16+up"] / F16_ERR_PARENT:.3f}; output scale {float(np.abs(g["out_grid"]).max()):.3g}')
    for name in ('x3+up', 'f16+up'):
        assert err['x3'] < err[name] < err['bf16'], err


@pytest.mark.parametrize('base', ['x3', 'f16'])
def test_batch_of_two_clips_equals_one_by_one(base, synth_weights):
    net = build(synth_weights, base, 'f16')
    x = torch.cat([synth.synth_clip(T=2, B=1, seed=1234), synth.synth_clip(T=2, B=1, seed=77, phase=1.0)], 0).cuda()
    both, aux = net(x, return_aux=True)
    for b in range(2):
        one, aux1 = net(x[b:b + 1], return_aux=True)
        assert torch.equal(aux1['indices'][0], aux['indices'][b])
        assert torch.equal(one[0], both[b])


def test_overflow_falls_back_to_the_exact_f32_kernels(synth_weights):
    """The input of tests/test_gpu_net_f16.py's fallback test: a counted fallback under x3 + knob, the result of the exact-f32 policy, and
    the knob back in force afterwards."""
    W = dict(synth_weights)
    W['ft_layers.4.linear1.weight'] = W['ft_layers.4.linear1.weight'] * 3.0e5
    W['ft_layers.4.linear2.weight'] = W['ft_layers.4.linear2.weight'] / 3.0e5
    x = synth.synth_clip(T=2, B=1, seed=21).cuda()
    n32, nup = build(W, 'fp32'), build(W, 'x3', 'f16')
    ref = n32(x)
    assert torch.isfinite(ref).all() and n32.x3_fallbacks == 0
    got = nup(x)
    assert nup.x3_fallbacks == 1 and nup.precision == 'x3' and nup.upsample_precision == 'f16'
    assert torch.equal(got, ref)
    assert nup.o.up2_x1 is True and nup.o.mma == L.MMA_X3      # the policy and the knob are back after the re-run


def test_back_to_the_default_computes_x3s_bits(synth_weights, monkeypatch):
    monkeypatch.delenv('KEEP_AMD_UPSAMPLE_PRECISION', raising=False)
    monkeypatch.delenv('KEEP_AMD_PRECISION', raising=False)
    x = synth.synth_clip(T=2, B=1, seed=1234).cuda()
    plain = KeepNet(**DEFAULT_ARCH)
    plain.load_state_dict(synth_weights, strict=True)
    plain.to('cuda').eval()
    assert plain.precision == 'x3' and plain.upsample_precision == 'x3'
    ref = plain(x)
    assert plain.o.up2_x1 is False and plain.o._up2_x1_route == {}
    net = build(synth_weights, 'x3', 'f16')
    moved = net(x)
    assert not torch.equal(moved, ref) and net.o._up2_x1_route
    net.set_upsample_precision('x3')
    assert torch.equal(net(x), ref) and net.o.up2_x1 is False


def test_knob_set_behind_a_replayed_graph_takes_effect_on_the_next_call(synth_weights):
    """B = 1 with hipGraph replay: the knob is part of the graph key, so a net that already replays its captured x3 forward runs (and then
    captures) the other kernel sequence on the next call -- the bits of an eager net that had the knob from the start."""
    x = synth.synth_clip(T=2, B=1, seed=1234).cuda()
    net = build(synth_weights, 'x3')
    net.graph_mode = '1'
    first = net(x).clone()
    again = net(x).clone()                      # a replay
    assert len(net._graphs) == 1 and torch.equal(first, again)
    net.set_upsample_precision('f16')
    net.o.census = census = {}
    try:
        moved = net(x).clone()
    finally:
        net.o.census = None
    assert census.get(ops.X1_UP2_KERNEL, 0) > 0 and X3_PHASES not in census
    assert len(net._graphs) == 2 and not torch.equal(moved, first)
    eager = build(synth_weights, 'x3', 'f16')
    eager.graph_mode = '0'
    assert torch.equal(eager(x), moved)
    assert torch.equal(net(x), moved)           # the replay of the second graph
