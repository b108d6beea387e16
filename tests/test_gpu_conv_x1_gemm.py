"""GPU suite (-m gpu): the single-fp16 (KEEP_MMA_X1) form of the GEMM variant of conv_x3_kernel, admitted by KEEP_CONV_X1_GEMM -- numerics
against fp64 with the derived bound of tests/test_gpu_parsenet_f16.py, batch invariance under per-image range scales, the fused max|out|,
the memory footprint in poisoned surroundings, and the x3 policy's indifference to the bit."""
import functools
import math

import pytest
import torch

import footprint as FP
from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu

X1_GEMM = {1: 'conv_x3_kernel<2, 2, 1, 1, true, 1, 0, 1, 0, 1>', 2: 'conv_x3_kernel<2, 2, 2, 2, true, 1, 0, 1, 0, 1>'}
# name -> geometry.  The smallest shapes at which the kernel can still go wrong:
#   ragged      35 rows per image (a 5 x 7 map), M = 70: a ragged 64-row block, Cout = 32 < the 64-wide tile, an out_ld = 48 slice write
#   one-step    M = 128, Cin = 32: a single K step (the prefetch ring never refills)
#   tile128     257 rows per image: 16 reference images x 257 > 4096 rows is the smallest count that plans the 128 x 128 tile; 16 real images
#               (M = 4112 = 32 x 128 + 16, above the 4096 rows up to which a launch runs the small tile) make the launch use it, with a ragged last block;
#               residual at res_ld = 272 and ReLU.  At that count the x3 rules split K 4 ways (66 blocks): bias / ReLU / residual run in the reduce
#   tile128-1p  1025 rows per image (odd, no multiple of 128): 16 reference images fill the chip, so the 128 x 128 tile runs in ONE pass and the
#               residual (res_ld = 272) + ReLU are its own epilogue's; 5 real images (M = 5125 > 4096, a ragged last block)
#   split-k     16 rows per image, Cin = 512, Cout = 64: 16 reference images give 4 blocks of 64 x 64 -> the plan splits K 8 ways; res_ld = 72
#   scales      two images of 64 rows whose magnitudes differ by 2^12 (per-image range scales of x3_in_amax), fused max|out|
CASES = {
    'ragged': dict(N=2, HW=35, Cin=64, Cout=32, out_ld=48, tile=1, split=1),
    'one-step': dict(N=2, HW=64, Cin=32, Cout=64, tile=1, split=1),
    'tile128': dict(N=16, HW=257, Cin=256, Cout=256, res_ld=272, act=L.ACT_RELU, tile=2, split=4),
    'tile128-1p': dict(N=5, HW=1025, Cin=256, Cout=256, res_ld=272, act=L.ACT_RELU, tile=2, split=1),
    'split-k': dict(N=2, HW=16, Cin=512, Cout=64, res_ld=72, act=L.ACT_RELU, tile=1, split=8),
    'scales': dict(N=2, HW=64, Cin=64, Cout=64, gains=(1.0, 2.0 ** 12), tile=1, split=1),
}


def in_scale(amax):
    """The power of two the kernels multiply an image by (keep_conv_common.h: x3_range_scale): amax * s in [2^14, 2^15)."""
    return 2.0 ** (14 - math.floor(math.log2(amax)))


@functools.lru_cache(maxsize=None)
def tensors(name):
    """Inputs of a case (built once, never modified): activations with the spread of test_gpu_parsenet_f16.spread_input -- a log-normal gain
    per (image, channel), sigma 1.2, and per row, sigma 0.5 -- weights with a per-(cout, cin) log-normal gain, bias, residual, the twins."""
    c = CASES[name]
    N, HW, Cin, Cout = c['N'], c['HW'], c['Cin'], c['Cout']
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = op_input(f'x1g_{name}', (N, HW, Cin)) * torch.exp(1.2 * torch.randn(N, 1, Cin, generator=g)) * torch.exp(0.5 * torch.randn(N, HW, 1, generator=g))
    for n, gain in enumerate(c.get('gains', ())):
        x[n] *= gain
    w = op_input(f'x1gw_{name}', (Cout, Cin), 1.0 / Cin ** 0.5) * torch.exp(0.7 * torch.randn(Cout, Cin, generator=g))
    b = op_input(f'x1gb_{name}', (Cout,), 0.1)
    res = op_input(f'x1gr_{name}', (N * HW, Cout)) if 'res_ld' in c else None
    sw = ops.x3_scale_for(float(w.abs().max()))
    t = dict(x=x.reshape(N * HW, Cin).contiguous(), w=w.contiguous(), b=b, res=res, sw=sw, amax=x.reshape(N, -1).abs().amax(1),
             wx1=(w * sw).to(torch.float16).contiguous(), wx3=ops.split_x3(w, sw).view(torch.int16).reshape(Cout, 2 * Cin).contiguous())
    return t


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64 result, sum |a w|, and the subnormal floor of the bound (see test_x1_gemm_numerics_against_fp64)."""
    c, t = CASES[name], tensors(name)
    N, HW, Cout = c['N'], c['HW'], c['Cout']
    x, w = t['x'].double(), t['w'].double()
    ref = x @ w.t() + t['b'].double()
    sabs = x.abs() @ w.abs().t()
    sa = torch.tensor([in_scale(float(a)) for a in t['amax']], dtype=torch.float64).repeat_interleave(HW).view(-1, 1)
    floor = (w.abs().sum(1).view(1, Cout) / sa + x.abs().sum(1, keepdim=True) / t['sw']) * 2.0 ** -25 * (1 + 2.0 ** -10)
    pre = ref.clone()
    if c.get('act') == L.ACT_RELU:
        ref = ref.clamp_min(0)
    rabs = torch.zeros_like(ref)
    if t['res'] is not None:
        ref = ref + t['res'].double()
        rabs = t['res'].double().abs()
    return ref, sabs, floor, pre.abs() + rabs


def make_args(name, t, mma, flags, N=None, split_k=0):
    c, tt = CASES[name], tensors(name)
    N = c['N'] if N is None else N
    return L.conv_args(inp=t['x'], weight=t['w'], bias=t['b'], out=t['out'], residual=t.get('res'), workspace=t.get('ws'),
                       N=N, H=c['HW'], W=1, Cin=c['Cin'], Cout=c['Cout'], KH=1, KW=1, stride=1, pad_t=0, pad_l=0, Ho=c['HW'], Wo=1, in_ld=c['Cin'],
                       out_ld=c.get('out_ld', c['Cout']), res_ld=c.get('res_ld', 0), epi_act=c.get('act', L.ACT_NONE), mma=mma,
                       weight_x3=t['wx1'] if mma == L.MMA_X1 else t['wx3'], x3_acc_scale=1.0 / tt['sw'], x3_in_amax=t['in_amax'],
                       x3_out_amax=t.get('amax'), flags=flags, split_k=split_k)


def host_plan(name, mma, flags, N=None):
    """The plan of a case before any buffer exists (keep_conv2d_plan looks at pointers only for their alignment)."""
    buf = torch.zeros(64, dtype=torch.float32)
    ptr = buf.data_ptr() // 16 * 16 + 16

    t = dict.fromkeys(('x', 'w', 'b', 'out', 'wx1', 'wx3', 'in_amax') + (('res',) if 'res_ld' in CASES[name] else ()), ptr)
    return L.conv2d_plan(make_args(name, t, mma, flags, N))


def regions(name, mma, flags, rows=None):
    """Every tensor of the launch as a footprint region.  ``rows``: (first image, one past the last) of a sub-batch."""
    c, t = CASES[name], tensors(name)
    n0, n1 = (0, c['N']) if rows is None else rows
    N, HW, Cin, Cout = n1 - n0, c['HW'], c['Cin'], c['Cout']
    pl = host_plan(name, mma, flags, N)
    sl = slice(n0 * HW, n1 * HW)
    tile = 128 * max(Cin, c.get('res_ld', Cout), c.get('out_ld', Cout)) * 4
    reg = [FP.single('x', t['x'][sl].contiguous(), tile_bytes=tile), FP.single('w', t['w']), FP.single('b', t['b'].reshape(1, -1)),
           FP.single('wx1' if mma == L.MMA_X1 else 'wx3', t['wx1'] if mma == L.MMA_X1 else t['wx3']),
           FP.single('in_amax', t['amax'][n0:n1].reshape(1, -1).contiguous()),
           FP.output('out', (N * HW, Cout), ld=c.get('out_ld'), off=8 if 'out_ld' in c else 0, tile_bytes=tile)]
    if t['res'] is not None:
        reg.append(FP.single('res', t['res'][sl].contiguous(), ld=c['res_ld'], off=4, tile_bytes=tile))
    if pl.out_amax_ok:
        reg.append(FP.output('amax', (1, N)))
    if pl.split_k > 1:
        assert pl.workspace_bytes == pl.split_k * N * HW * Cout * 4
        reg.append(FP.output('ws', (pl.split_k * N * HW, Cout), tile_bytes=tile, compare=False))
    return reg, pl, N


def launcher(name, mma, flags, N):
    def launch(t):
        a = make_args(name, t, mma, flags, N)
        pl = L.conv2d_plan(a)
        a.split_k = pl.split_k
        L.conv2d_launch(a)
        return pl.kernel.decode(), pl.split_k
    return launch


@functools.lru_cache(maxsize=None)
def plain_run(name, mma, flags, rows=None):
    reg, pl, N = regions(name, mma, flags, rows)
    out, sig = FP.plain(launcher(name, mma, flags, N), reg, 'cuda')
    return {k: v.cpu() for k, v in out.items()}, sig, pl


@pytest.mark.parametrize('name', list(CASES))
def test_x1_gemm_numerics_against_fp64(name):
    """Each operand is multiplied by an exact power of two and rounded once to fp16 (<= 2^-11 relative each inside the normal range), the
    fp32 accumulation of K terms (in split-K partials or not: the reduce adds split_k << K more roundings) adds <= K 2^-24 of sum |a w|:

        |err| <= (2^-10 + 2^-22 + K 2^-24) sum |a w|  +  floor  +  2^-22 (|acc + bias| + |residual|)

    floor: scaled operands below 2^-14 are rounded on the subnormal grid, sum_k (|w_k| / s_a + |a_k| / s_w) 2^-25 (1 + 2^-10) with the
    image's range scale s_a and the tensor's weight scale s_w.  Last term: the fp32 roundings of the epilogue (bias add, residual add, store;
    ReLU is exact).  Nothing here is measured."""
    c = CASES[name]
    out, (kernel, split_k), pl = plain_run(name, L.MMA_X1, L.CONV_X1_GEMM)
    assert kernel == X1_GEMM[c['tile']] and split_k == c['split'], (kernel, split_k)
    ref, sabs, floor, epi = reference(name)
    got = out['out'].double()
    bound = (2.0 ** -10 + 2.0 ** -22 + c['Cin'] * 2.0 ** -24) * sabs + floor + 2.0 ** -22 * (epi + tensors(name)['b'].double().abs())
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    print(f'[x1-gemm] {name}: {kernel} split {split_k}; max err {float(err.max()):.3e} (|ref| max {float(ref.abs().max()):.3g}), worst err / bound {ratio:.3f}, '
          f'floor share {float((floor / bound).max()):.2e}')
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (name, ratio)
    if pl.out_amax_ok:                  # the fused max |out| == max |out| of the written tensor, per image
        assert torch.equal(out['amax'].reshape(-1), out['out'].reshape(c['N'], -1).abs().amax(1))
    else:
        assert 'amax' not in out
    # the x1 kernel, not a quiet change of policy: away from x3's fp32-grade result by an fp16 rounding's worth
    o3 = plain_run(name, L.MMA_X3, 0)[0]['out']
    assert float((o3 - out['out']).abs().max()) > 2.0 ** -16 * float(sabs.max()) * 1e-2
    assert float((o3.double() - ref).abs().div(bound).max()) < ratio


def test_fused_amax_case_is_planned_with_it():
    assert plain_run('scales', L.MMA_X1, L.CONV_X1_GEMM)[2].out_amax_ok == 1
    assert plain_run('one-step', L.MMA_X1, L.CONV_X1_GEMM)[2].out_amax_ok == 1
    assert plain_run('ragged', L.MMA_X1, L.CONV_X1_GEMM)[2].out_amax_ok == 0      # 35 rows per image: a wave's rows straddle two images


@pytest.mark.parametrize('name', ['scales', 'ragged', 'split-k'])
def test_batch_equals_one_by_one(name):
    """Per-image range scales (two images 2^12 apart), images that share a row block, split-K planned from the reference batch: a frame's
    bits do not depend on its batch-mates."""
    c = CASES[name]
    both, sig, _ = plain_run(name, L.MMA_X1, L.CONV_X1_GEMM)
    for n in range(c['N']):
        one, sig1, _ = plain_run(name, L.MMA_X1, L.CONV_X1_GEMM, (n, n + 1))
        assert sig1 == sig
        assert torch.equal(one['out'].view(torch.int32), both['out'][n * c['HW']:(n + 1) * c['HW']].view(torch.int32)), (name, n)
        if 'amax' in both:
            assert torch.equal(one['amax'].reshape(-1), both['amax'].reshape(-1)[n:n + 1])


@pytest.mark.parametrize('name', list(CASES))
def test_x1_gemm_memory_footprint(name):
    """The same launches in poisoned surroundings (tests/footprint.py): nothing outside the declared outputs (the out_ld slice, the max|out|
    slots, the split-K workspace) changes, no result depends on bytes outside the inputs' payloads (the res_ld gap columns, rows past M), and
    the embedded call equals the plain one bit for bit."""
    reg, pl, N = regions(name, L.MMA_X1, L.CONV_X1_GEMM)
    out = FP.run(launcher(name, L.MMA_X1, L.CONV_X1_GEMM, N), reg, 'cuda')
    assert torch.equal(out['out'].cpu().view(torch.int32), plain_run(name, L.MMA_X1, L.CONV_X1_GEMM)[0]['out'].view(torch.int32))


@pytest.mark.parametrize('name', ['ragged', 'tile128', 'tile128-1p'])
def test_x3_ignores_the_bit(name):
    """KEEP_MMA_X3 with KEEP_CONV_X1_GEMM set: the same plan and the same bits as without it (recorded from the x3 kernel in this run)."""
    recorded, sig0, _ = plain_run(name, L.MMA_X3, 0)
    flagged, sig1, _ = plain_run(name, L.MMA_X3, L.CONV_X1_GEMM)
    assert sig0 == sig1 and sig0[0].startswith('conv_x3_kernel<') and sig0[0].endswith('true, true>'), (sig0, sig1)
    assert torch.equal(recorded['out'].view(torch.int32), flagged['out'].view(torch.int32))
    assert torch.isfinite(recorded['out']).all()


def test_without_the_bit_the_launch_is_refused():
    reg, _, N = regions('one-step', L.MMA_X1, L.CONV_X1_GEMM)
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1 has no kernel for this call'):
        FP.plain(launcher('one-step', L.MMA_X1, 0, N), reg, 'cuda')
