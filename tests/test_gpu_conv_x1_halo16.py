"""GPU suite (-m gpu): the single-fp16 (KEEP_MMA_X1) form of the 16 x 16-tile halo kernel, admitted by KEEP_CONV_X1_HALO16, through the C ABI --
numerics against fp64 with a derived bound, the single rounding (it is not the x3 kernel), batch invariance and the memory footprint in
poisoned surroundings."""
import functools
import itertools
import math

import pytest
import torch

import footprint as FP
from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu

X1_HALO16 = {L.ACT_NONE: 'conv3x3_halo_x3_kernel<16, 0, true, true, true, false, true>',
             L.ACT_SILU: 'conv3x3_halo_x3_kernel<16, 0, false, true, true, false, true>'}
# the form is admitted where KEEP_MMA_X3 plans the call un-split: 256 reference images put >= 256 items on every map below (a caller setting,
# never the real N); it stays fixed through every test of this file
REF_IMAGES = 256
N = 2
MAPS = ((16, 16), (32, 48))             # one tile / six tiles (2 x 3: tile rows and columns that are inner, top / bottom and left / right edges)
CINS = (32, 96)                         # one 32-channel chunk (the prefetch never refills) / three
COUTS = (48, 128)                       # a ragged 64-cout block / two whole ones
RES_LD, OUT_LD, OUT_OFF = 136, 144, 8   # residual rows and the wider output tensor the slice is written into
CASES = list(itertools.product(MAPS, CINS, COUTS, (False, True), (L.ACT_NONE, L.ACT_SILU), (False, True)))


def case_id(c):
    (H, W), Cin, Cout, res, act, amax = c
    return f"{H}x{W}-ci{Cin}-co{Cout}-{'res+slice' if res else 'plain'}-{'silu' if act else 'none'}-{'amax' if amax else 'noamax'}"


def in_scale(amax):
    """The power of two the kernels multiply an image by (keep_conv_common.h: x3_range_scale): amax * s in [2^14, 2^15)."""
    return 2.0 ** (14 - math.floor(math.log2(amax)))


@functools.lru_cache(maxsize=None)
def tensors(hw, Cin, Cout):
    """Inputs of a geometry (built once, never modified; three images, the tests take the first N = 2 and the batch test 1 and 3): activations with a log-normal gain per (image, channel), sigma 1.2, image 1 another
    2^3 up (per-image range scales differ), weights with a per-(cout, cin) log-normal gain, bias, residual, the two twins."""
    H, W = hw
    tag = f'{H}x{W}_{Cin}_{Cout}'
    g = torch.Generator().manual_seed(1000 * H + 10 * Cin + Cout)
    x = op_input(f'x1h_{tag}', (3, H, W, Cin)) * torch.exp(1.2 * torch.randn(3, 1, 1, Cin, generator=g))
    x[1] *= 8.0
    w = op_input(f'x1hw_{tag}', (Cout, 3, 3, Cin), 1.0 / (9 * Cin) ** 0.5) * torch.exp(0.7 * torch.randn(Cout, 1, 1, Cin, generator=g))
    b = op_input(f'x1hb_{tag}', (Cout,), 0.1)
    res = op_input(f'x1hr_{tag}', (3, H, W, Cout))
    sw = ops.x3_scale_for(float(w.abs().max()))
    return dict(x=x.contiguous(), w=w.contiguous(), b=b, res=res.contiguous(), sw=sw, amax=x.reshape(3, -1).abs().amax(1),
                wx1=(w * sw).to(torch.float16).reshape(Cout, 9 * Cin).contiguous(),
                wx3=ops.split_x3(w.reshape(Cout * 9, Cin), sw).view(torch.int16).reshape(Cout, 18 * Cin).contiguous())


@functools.lru_cache(maxsize=None)
def conv64(hw, Cin, Cout):
    """fp64 convolution of the fp32 inputs (+ bias), sum |a| |w|, sum |a| and sum |w| over the 3 x 3 x Cin window of every output."""
    t = tensors(hw, Cin, Cout)
    x = t['x'][:N].double().permute(0, 3, 1, 2)
    w = t['w'].double().permute(0, 3, 1, 2)
    F = torch.nn.functional
    y = F.conv2d(x, w, t['b'].double(), padding=1).permute(0, 2, 3, 1)
    sabs = F.conv2d(x.abs(), w.abs(), padding=1).permute(0, 2, 3, 1)
    asum = F.conv2d(x.abs(), torch.ones(1, Cin, 3, 3, dtype=torch.float64), padding=1).permute(0, 2, 3, 1)
    wsum = w.abs().sum((1, 2, 3)).view(1, 1, 1, Cout)
    return y.contiguous(), sabs.contiguous(), asum.contiguous(), wsum


def make_args(c, t, mma, n=N, flags=L.CONV_X1_HALO16):
    (H, W), Cin, Cout, res, act, amax = c
    tt = tensors((H, W), Cin, Cout)
    return L.conv_args(inp=t['x'], weight=t['w'], bias=t['b'], out=t['out'], residual=t.get('res'), N=n, H=H, W=W, Cin=Cin, Cout=Cout, KH=3, KW=3,
                       stride=1, pad_t=1, pad_l=1, Ho=H, Wo=W, in_ld=Cin, out_ld=OUT_LD if res else Cout, res_ld=RES_LD if res else 0, epi_act=act,
                       mma=mma, weight_x3=t['wx1'] if mma == L.MMA_X1 else t['wx3'], x3_acc_scale=1.0 / tt['sw'],
                       x3_in_amax=t['in_amax'] if amax else None, flags=flags, plan_ref_images=REF_IMAGES)


def regions(c, mma, n=N):
    (H, W), Cin, Cout, res, act, amax = c
    t = tensors((H, W), Cin, Cout)
    tile = 18 * 18 * max(Cin, OUT_LD) * 4
    reg = [FP.single('x', t['x'][:n].reshape(n * H * W, Cin).contiguous(), tile_bytes=tile), FP.single('w', t['w'].reshape(Cout, 9 * Cin)),
           FP.single('b', t['b'].reshape(1, -1)), FP.single('wx1' if mma == L.MMA_X1 else 'wx3', t['wx1'] if mma == L.MMA_X1 else t['wx3']),
           FP.output('out', (n * H * W, Cout), ld=OUT_LD if res else None, off=OUT_OFF if res else 0, tile_bytes=tile)]
    if amax:
        reg.append(FP.single('in_amax', t['amax'][:n].reshape(1, -1).contiguous()))
    if res:
        reg.append(FP.single('res', t['res'][:n].reshape(n * H * W, Cout).contiguous(), ld=RES_LD, off=4, tile_bytes=tile))
    return reg


def launcher(c, mma, n=N):
    def launch(t):
        a = make_args(c, t, mma, n)
        pl = L.conv2d_plan(a)
        assert pl.workspace_bytes == 0
        a.split_k = pl.split_k
        L.conv2d_launch(a)
        return pl.kernel.decode(), pl.split_k
    return launch


@functools.lru_cache(maxsize=None)
def plain_run(c, mma, n=N):
    out, sig = FP.plain(launcher(c, mma, n), regions(c, mma, n), 'cuda')
    return out['out'].cpu(), sig


WORST = {}


@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_x1_halo16_numerics_against_fp64(c):
    """Each operand is multiplied by an exact power of two and rounded ONCE to fp16 -- 11 significant bits, <= 2^-11 relative each, so a
    product is off by <= 2 * 2^-11 + 2^-22 -- and the K = 9 Cin products are accumulated in fp32 (<= K 2^-24 of sum |a| |w|, the term of the
    x3-vs-fp64 tests):

        |acc - acc64| <= (2^-10 + 2^-22 + K 2^-24) sum |a| |w|  +  floor,      floor = (sum |w| / s_a + sum |a| / s_w) 2^-25 (1 + 2^-10)

    floor: scaled operands below 2^-14 land on fp16's subnormal grid (s_a the image's range scale -- 1 without x3_in_amax --, s_w the weight
    tensor's).  The epilogue: bias add and store round in fp32 (2^-22 (|acc + bias| + |bias|)); the fast SiLU (x3 grade: v_exp / v_rcp forms,
    relative 2^-20) has slope <= 1.1, so it passes 1.1 x the accumulator error on; the residual add rounds once more.  Nothing is measured."""
    hw, Cin, Cout, res, act, amax = c
    t = tensors(hw, Cin, Cout)
    got, (kernel, split_k) = plain_run(c, L.MMA_X1)
    assert kernel == X1_HALO16[act] and split_k == 1, (kernel, split_k)
    y, sabs, asum, wsum = conv64(hw, Cin, Cout)
    sa = torch.tensor([in_scale(float(a)) if amax else 1.0 for a in t['amax'][:N]], dtype=torch.float64).view(N, 1, 1, 1)
    floor = (wsum / sa + asum / t['sw']) * 2.0 ** -25 * (1 + 2.0 ** -10)
    bound = (2.0 ** -10 + 2.0 ** -22 + 9 * Cin * 2.0 ** -24) * sabs + floor + 2.0 ** -22 * (y.abs() + t['b'].double().abs())
    ref = y
    if act == L.ACT_SILU:
        ref = y * torch.sigmoid(y)
        bound = 1.1 * bound + 2.0 ** -20 * ref.abs() + 2.0 ** -126
    if res:
        ref = ref + t['res'][:N].double()
        bound = bound + 2.0 ** -23 * (ref.abs() + t['res'][:N].double().abs())
    got = got.view(N, hw[0], hw[1], Cout).double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    # single rounding, not x3: the x3 policy on the same case is closer to fp64 by orders of magnitude, and this result is off by an fp16
    # rounding's worth on at least one element
    o3, sig3 = plain_run(c, L.MMA_X3)
    e3 = (o3.view(got.shape).double() - ref).abs()
    WORST[case_id(c)] = ratio
    print(f'[x1-halo16] {case_id(c)}: {kernel}; max err {float(err.max()):.3e} (x3 {sig3[0]}: {float(e3.max()):.3e}; |ref| max {float(ref.abs().max()):.3g}), '
          f'worst err / bound {ratio:.3f} (x3: {float((e3 / bound).max()):.2e}), floor share {float((floor / bound).max()):.2e}')
    assert ratio <= 1.0, (case_id(c), ratio)
    assert 'X1' not in sig3[0] and not sig3[0].endswith('false, true>')
    assert bool((err > 16 * e3 + 2.0 ** -16 * sabs * 1e-2).any()), 'no element sits an order of magnitude above the x3 kernel: not the single-fp16 form'
    assert float(e3.max()) < float(err.max()) / 16


@pytest.mark.parametrize('c', [c for c in CASES if c[1] == 96 and c[2] == 128 and c[4] == L.ACT_SILU], ids=case_id)
def test_batch_invariance(c):
    """Image 0 of an N = 1 call equals image 0 of an N = 3 call bit for bit (plan_ref_images fixed; with x3_in_amax the images' range scales
    differ by 2^3): the plan follows the reference batch and a block's sums never cross images."""
    hw = c[0]
    outs = {n: FP.plain(launcher(c, L.MMA_X1, n), regions(c, L.MMA_X1, n), 'cuda') for n in (1, 3)}
    outs = {n: (o['out'].cpu(), sig) for n, (o, sig) in outs.items()}
    hwn = hw[0] * hw[1]
    assert outs[1][1] == outs[3][1]
    assert torch.equal(outs[1][0][:hwn].view(torch.int32), outs[3][0][:hwn].view(torch.int32))
    assert torch.isfinite(outs[3][0]).all()


@pytest.mark.parametrize('c', [((32, 48), 96, 48, True, L.ACT_SILU, True), ((16, 16), 32, 128, False, L.ACT_NONE, False)], ids=case_id)
def test_x1_halo16_memory_footprint(c):
    """The launch in poisoned surroundings (tests/footprint.py): nothing before or after the `out` slice and none of the untouched columns of
    the wider out_ld tensor changes (Cout = 48: the cout rows 48 .. 63 of the block are never stored), no result depends on bytes outside
    the inputs' payloads (halo pixels outside the image, the res_ld gap columns), and the embedded call equals the plain one bit for bit."""
    out = FP.run(launcher(c, L.MMA_X1), regions(c, L.MMA_X1), 'cuda')
    assert torch.equal(out['out'].cpu().view(torch.int32), plain_run(c, L.MMA_X1)[0].view(torch.int32))


def test_without_the_bit_the_launch_is_refused():
    c = ((16, 16), 32, 128, False, L.ACT_NONE, False)

    def launch(t):
        a = make_args(c, t, L.MMA_X1, flags=0)
        L.conv2d_launch(a)
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1 has no kernel for this call'):
        FP.plain(launch, regions(c, L.MMA_X1), 'cuda')
