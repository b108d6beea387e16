"""keep_gm_ffn_x1 (csrc/keep_ffn_x3.hip, include/keep_cv_hip.h): GMFlow's fused feed-forward block on single-fp16 operands, as a kernel --
against a float64 twin computed on the operands the kernel rounds, against the unrounded float64 reference beside the x3 entry and a
bf16 twin, and its memory footprint under poisoned surroundings.

The inputs have the scales of test_gm_ffn_x3_fused_kernel (src 1.5 N(0,1), msg N(0,1), W0 0.08 N(0,1), W2 0.05 N(0,1), gamma
1 + 0.3 N(0,1), beta 0.2 N(0,1)), drawn with torch.randn from this file's own seeds.  The references are computed once per shape on the
CPU and shared by the exact_act = 0 / 1 cases; test_the_references_alone_keep_the_two_bounds (no GPU) checks that the references by
themselves stay inside the bounds the kernel is held to."""
import functools

import pytest
import torch

import footprint as FP
import test_gpu_footprint as T
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

C = 128
# (M, hidden): one row in a ragged block; one block, one chunk, no prefetch; one row in the second block and an odd chunk count (both LDS
# stages, the stage parity); the workload's hidden width with a ragged tail
SHAPES = [(1, 1024), (256, 32), (257, 96), (777, 1024)]


def _gelu64(h):
    return 0.5 * h * (1.0 + torch.erf(h / 2.0 ** 0.5))


@functools.lru_cache(maxsize=None)
def case(M, hidden):
    """Inputs, twins and references of one shape (CPU, float64 unless said): computed once, never modified."""
    g_ = torch.Generator().manual_seed(1000 * hidden + M)
    r = lambda *s: torch.randn(*s, generator=g_)
    src, msg = 1.5 * r(M, C), 1.0 * r(M, C)
    w0, w2 = 0.08 * r(hidden, 2 * C), 0.05 * r(C, hidden)
    gamma, beta = 1.0 + 0.3 * r(C), 0.2 * r(C)
    w2p = ops.ffn_w2_perm(w2)
    s0, s2 = ops.x3_scale_for(float(w0.abs().max())), ops.x3_scale_for(float(w2p.abs().max()))

    def tail(hmid, w2_used):
        y = hmid @ w2_used.double().t()
        return torch.nn.functional.layer_norm(y, (C,), gamma.double(), beta.double(), 1e-5) + src.double()

    x = torch.cat([src, msg], 1)
    ref = tail(_gelu64(x.double() @ w0.double().t()), w2)

    def twin(dt, acc32=False):
        """X, W0 * 2^e, gelu(h) and W2 * 2^e rounded to ``dt``; everything else float64 (``acc32``: h summed in float32, as a kernel does)."""
        xr, w0r = x.to(dt), (w0 * s0).to(dt)
        h = (xr.float() @ w0r.float().t()).double() if acc32 else xr.double() @ w0r.double().t()
        hr = _gelu64(h / s0).float().to(dt)      # (the kernel rounds an fp32 GELU value: round the float32 of it)
        return tail(hr.double(), (w2 * s2).to(dt).double() / s2)      # (the permutation only reorders W2's columns and the matching K slots)

    t64 = twin(torch.float16)
    d_flip = float((twin(torch.float16, acc32=True) - t64).abs().max())
    err_f16twin = float((t64 - ref).abs().max())
    err_bf16twin = float((twin(torch.bfloat16) - ref).abs().max())
    return dict(src=src, msg=msg, w0=w0, w2=w2, w2p=w2p, s0=s0, s2=s2, gamma=gamma, beta=beta, ref=ref, twin64=t64, d_flip=d_flip,
                err_f16twin=err_f16twin, err_bf16twin=err_bf16twin)


@pytest.mark.parametrize('M,hidden', SHAPES)
def test_the_references_alone_keep_the_two_bounds(M, hidden):
    """No GPU: the fp16 twin itself is within 0.25 x the bf16 twin's error (three more mantissa bits predict 1 / 8), and the twin's
    sensitivity to rounding flips is small against the outputs' scale, so a layout or permutation error shows at O(1)."""
    c = case(M, hidden)
    print(f'[ffn-x1 ref] M={M} hidden={hidden}: d_flip {c["d_flip"]:.3e}, fp16 twin {c["err_f16twin"]:.3e}, bf16 twin {c["err_bf16twin"]:.3e}, '
          f'ratio {c["err_f16twin"] / c["err_bf16twin"]:.3f}, |ref| max {float(c["ref"].abs().max()):.3g}')
    assert c['err_f16twin'] <= 0.25 * c['err_bf16twin']
    assert 4 * c['d_flip'] + 2e-4 < 1e-2 < float(c['ref'].abs().max())


def _x1_twins(c):
    return ((c['w0'] * c['s0']).to(torch.float16).view(torch.int16).cuda(), (c['w2p'] * c['s2']).to(torch.float16).view(torch.int16).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize('exact_act', [0, 1])
@pytest.mark.parametrize('M,hidden', SHAPES)
def test_gm_ffn_x1_kernel_against_fp64(M, hidden, exact_act):
    c = case(M, hidden)
    sd, md, gd, bd = c['src'].cuda(), c['msg'].cuda(), c['gamma'].cuda(), c['beta'].cuda()
    w0x1, w2x1 = _x1_twins(c)
    guard = torch.full((64, C), 123.0, device='cuda')
    out = torch.cat([torch.full((M, C), float('nan'), device='cuda'), guard])
    L.call('keep_gm_ffn_x1', sd, md, w0x1, 1.0 / c['s0'], w2x1, 1.0 / c['s2'], gd, bd, 1e-5, out, M, C, hidden, exact_act)
    # 1. rows behind M are untouched
    assert torch.equal(out[M:], guard)
    got = out[:M].double().cpu()
    assert torch.isfinite(got).all()
    # the x3 entry in the same run
    w0x3, w2x3 = ops.split_x3(c['w0'], c['s0']).cuda(), ops.split_x3(c['w2p'], c['s2']).cuda()
    out3 = torch.empty((M, C), device='cuda')
    L.call('keep_gm_ffn_x3', sd, md, w0x3, 1.0 / c['s0'], w2x3, 1.0 / c['s2'], gd, bd, 1e-5, out3, M, C, hidden, exact_act)
    err_twin = float((got - c['twin64']).abs().max())
    err_x1 = float((got - c['ref']).abs().max())
    err_x3 = float((out3.double().cpu() - c['ref']).abs().max())
    print(f'[ffn-x1] M={M} hidden={hidden} exact_act={exact_act}: |kernel - twin64| {err_twin:.3e} (d_flip {c["d_flip"]:.3e}), err_x1 {err_x1:.3e}, '
          f'err_x3 {err_x3:.3e}, err_bf16twin {c["err_bf16twin"]:.3e}, err_x1 / err_bf16twin {err_x1 / c["err_bf16twin"]:.3f}')
    # 2. the float64 twin on rounded operands
    assert err_twin <= 4 * c['d_flip'] + 2e-4, (err_twin, c['d_flip'])
    # 3. the unrounded float64 reference: really single fp16, and three mantissa bits better than bf16
    assert err_x1 >= 20 * err_x3, (err_x1, err_x3)
    assert err_x1 <= 0.25 * c['err_bf16twin'], (err_x1, c['err_bf16twin'])
    # 4. refusals from Python
    with pytest.raises(L.KeepHipError, match='keep_gm_ffn_x1'):
        L.call('keep_gm_ffn_x1', sd, md, w0x1, 1.0 / c['s0'], w2x1, 1.0 / c['s2'], gd, bd, 1e-5, out, M, 64, hidden, exact_act)


# ------------------------------------------------------------------------------------------------ footprint
def _gm_ffn_x1(m, hidden, eps=1e-5, exact_act=0):
    """The keep_gm_ffn_x3 footprint case with the hi-only twins: the same plain weights and inputs."""
    w0, w2 = T.gm_ffn_weights(hidden, C)
    w2 = ops.ffn_w2_perm(w2)
    s0, s2 = ops.x3_scale_for(float(w0.abs().max())), ops.x3_scale_for(float(w2.abs().max()))
    w0x, w2x = (w0 * s0).to(torch.float16).view(torch.int16), (w2 * s2).to(torch.float16).view(torch.int16)
    R = [T._in('src', T.rnd('fs', (m, C))), T._in('msg', T.rnd('fm', (m, C))), T._in('w0', w0x.reshape(hidden, -1)), T._in('w2', w2x.reshape(C, -1)),
         T._in('g', T.rnd('fg', (1, C)) * 0.2 + 1), T._in('b', T.rnd('fb', (1, C)) * 0.2), FP.output('o', (m, C))]
    return R, lambda t: L.call('keep_gm_ffn_x1', t['src'], t['msg'], t['w0'], 1.0 / s0, t['w2'], 1.0 / s2, t['g'], t['b'], eps, t['o'], m, C, hidden, exact_act)


@pytest.mark.gpu
@pytest.mark.parametrize('case_id,m,hidden', [('aligned', 256, 256), ('ragged', 777, 96)])
def test_gm_ffn_x1_footprint(case_id, m, hidden):
    regions, launch = _gm_ffn_x1(m, hidden)
    FP.run(launch, regions, 'cuda')
