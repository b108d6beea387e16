"""GPU suite (-m gpu): the KEEP network's opt-in single-fp16 precision ('f16': x3 with KEEP_MMA_X1 on the streaming 3x3 convolutions) --
routing by the library's plan, quality against the reference golden beside 'bf16', batch invariance, the fp16-range fallback and the
untouched default.  Every test builds its own network (the session's `gpu_net` fixture keeps its two policies)."""
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

# max |pixel - reference| on the T = 3 golden's 32 x 32 digest with the reference's indices injected, precision 'f16', on the first green
# run (MI355X, 2026-10-17): see F16_ERR_MEASURED.  The test allows twice that (reduction order of the statistics kernels from
# box to box) and demands strictly less than 'bf16' measured in the same run.  Not the 1e-3 parity tolerance: this mode is outside it.
F16_ERR_MEASURED = 3.5299e-03      # (same run: bf16 4.0754e-02, x3 1.3903e-05; output scale 1.01)
X1_SWISH = 'conv3x3_halo_x3s_kernel<1, true, true>'
X1_FORMS = ('conv3x3_halo_x3s_kernel<0, false, true>', 'conv3x3_halo_x3s_kernel<0, true, true>', X1_SWISH, 'conv3x3_halo_x3s_kernel<2, true, true>')


def build(weights, precision):
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(weights, strict=True)
    return net.to('cuda').eval().set_precision(precision)


def digest(frames):
    T, C, H, Wd = frames.shape
    return frames[:, :, 7::H // 32, 5::Wd // 32][:, :, :32, :32]


@pytest.fixture(scope='module')
def f16_net(synth_weights):
    return build(synth_weights, 'f16')


def test_f16_routes_the_prologue_convolutions_to_x1_and_everything_else_to_x3(f16_net, synth_weights):
    """The launch census of one T = 2 forward, read through keep_conv2d_plan's kernel names: the GroupNorm-swish 3x3 layers run the X1
    swish instantiation, no x3 streaming launch is left where the library admits X1, and every other kernel family is exactly what the
    x3 policy launches (same names, same counts).  Attention is an x3 launch (Ops.attn_mma)."""
    x = synth.synth_clip(T=2, B=1, seed=1234).cuda()
    census = {}
    for pol, net in (('f16', f16_net), ('x3', build(synth_weights, 'x3'))):
        net.o.census = census[pol] = {}
        try:
            out = net(x)
        finally:
            net.o.census = None
        assert torch.isfinite(out).all()
    c16, c3 = census['f16'], census['x3']
    print('[f16-census] f16:', sorted(c16.items()), '\n[f16-census] x3 :', sorted(c3.items()))
    assert f16_net.o.mma == L.MMA_X3 and f16_net.o.attn_mma == L.MMA_X3 and f16_net.o.blobx1 is not None
    assert c16.get(X1_SWISH, 0) > 0
    x1 = sum(n for k, n in c16.items() if k in X1_FORMS)
    assert all(k in X1_FORMS for k in c16 if k.endswith('true>') and k.startswith('conv3x3_halo_x3s_kernel<'))
    # every launch that left the x3 streaming kernel arrived at an X1 form; nothing else moved
    assert c3[ops.X3_STREAM_KERNEL] - c16.get(ops.X3_STREAM_KERNEL, 0) == x1
    rest16 = {k: n for k, n in c16.items() if k not in X1_FORMS and k != ops.X3_STREAM_KERNEL}
    rest3 = {k: n for k, n in c3.items() if k != ops.X3_STREAM_KERNEL}
    assert rest16 == rest3
    assert not any(k in X1_FORMS for k in c3)
    # what stays on the x3 streaming kernel under f16 is what the library has no X1 kernel for (GMFlow's twins are not built)
    assert c16.get(ops.X3_STREAM_KERNEL, 0) < c3[ops.X3_STREAM_KERNEL]


def test_f16_against_the_reference_golden_beside_bf16(f16_net, synth_weights):
    g = np.load(os.path.join(GOLDEN, 'keep_forward_T3.npz'))
    x = synth.synth_clip(T=3, B=1, seed=1234).cuda()
    forced = torch.from_numpy(g['indices'].astype(np.int32)).view(1, 3, -1)
    err = {}
    for pol, net in (('f16', f16_net), ('bf16', build(synth_weights, 'bf16')), ('x3', build(synth_weights, 'x3'))):
        out = net(x, force_indices=forced)
        assert torch.isfinite(out).all()
        err[pol] = float(np.abs(digest(out[0].cpu()).numpy() - g['out_grid']).max())
    print(f'[f16-golden] max-abs pixel error, reference indices injected (T = 3): f16 {err["f16"]:.4e}, bf16 {err["bf16"]:.4e}, x3 {err["x3"]:.4e}; '
          f'output scale {float(np.abs(g["out_grid"]).max()):.3g}')
    assert f16_net.x3_fallbacks == 0
    assert err['f16'] < err['bf16']
    assert err['f16'] > err['x3']                  # really the single-fp16 kernels
    assert F16_ERR_MEASURED is not None, f'F16_ERR_MEASURED not recorded yet; measured {err}'
    assert err['f16'] <= 2.0 * F16_ERR_MEASURED, err


def test_f16_batch_of_two_clips_equals_one_by_one(f16_net):
    x = torch.cat([synth.synth_clip(T=2, B=1, seed=1234), synth.synth_clip(T=2, B=1, seed=77, phase=1.0)], 0).cuda()
    both, aux = f16_net(x, return_aux=True)
    for b in range(2):
        one, aux1 = f16_net(x[b:b + 1], return_aux=True)
        assert torch.equal(aux1['indices'][0], aux['indices'][b])
        assert torch.equal(one[0], both[b])


def test_f16_overflow_falls_back_to_the_exact_f32_kernels(synth_weights):
    """The input of tests/test_gpu_net.py::test_x3_overflow_on_the_index_chain_falls_back_to_f32: one transformer MLP weight scaled so that
    gelu(linear1) leaves the fp16 range -- a counted fallback under 'f16', and the result of the exact-f32 policy."""
    W = dict(synth_weights)
    W['ft_layers.4.linear1.weight'] = W['ft_layers.4.linear1.weight'] * 3.0e5
    W['ft_layers.4.linear2.weight'] = W['ft_layers.4.linear2.weight'] / 3.0e5
    x = synth.synth_clip(T=2, B=1, seed=21).cuda()
    n32, n16 = build(W, 'fp32'), build(W, 'f16')
    ref = n32(x)
    assert torch.isfinite(ref).all() and n32.x3_fallbacks == 0
    got = n16(x)
    assert n16.x3_fallbacks == 1 and n16.precision == 'f16'
    assert torch.equal(got, ref)
    assert n16.o.blobx1 is not None and n16.o.mma == L.MMA_X3      # the policy is back after the re-run


def test_default_is_x3_and_bit_equal_to_a_net_that_never_built_an_x1_twin(synth_weights, monkeypatch):
    monkeypatch.delenv('KEEP_AMD_PRECISION', raising=False)
    x = synth.synth_clip(T=2, B=1, seed=1234).cuda()
    plain = KeepNet(**DEFAULT_ARCH)
    plain.load_state_dict(synth_weights, strict=True)
    plain.to('cuda').eval()
    assert plain.precision == 'x3'
    ref = plain(x)
    assert plain._dev_blobx1 is None and plain.o.blobx1 is None
    # a net that ran 'f16' (twin built) and went back to the default computes the same bits
    net = build(synth_weights, 'f16')
    net(x)
    assert net._dev_blobx1 is not None
    net.set_precision('x3')
    assert torch.equal(net(x), ref) and net.o.blobx1 is None
