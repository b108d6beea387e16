"""GPU suite (-m gpu): the single-fp16 streaming 3x3 kernel behind a GroupNorm prologue (KEEP_MMA_X1 + pro_scale / pro_shift, alone, with
ReLU, with swish: conv3x3_halo_x3s_kernel<PRO, true, true>, ABI v23) -- numerics against fp64 from once-rounded operands, zero padding
behind a shifting affine, the fused GroupNorm partials, the memory footprint and the library's plan."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import footprint as FP
from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu

PRO_NAME = {L.PRO_NONE: 'affine', L.PRO_RELU: 'affine+relu', L.PRO_SWISH: 'affine+swish'}
X1_PRO_KERNEL = {L.PRO_NONE: 'conv3x3_halo_x3s_kernel<0, true, true>', L.PRO_SWISH: 'conv3x3_halo_x3s_kernel<1, true, true>',
                 L.PRO_RELU: 'conv3x3_halo_x3s_kernel<2, true, true>'}

# (id, N, Cin, Cout, H, W, prologue, epilogue variant, nearest-x2 input).  Cin 32: one weight row serves both chunks of the item; 64: two
# rows.  Cout 96: a ragged second 64-cout block.  8 x 32: one tile, every halo pixel is padding; 16 x 64: four tiles, real neighbours on both
# axes.  Every prologue meets every map size and both Cin; every epilogue variant appears with the swish (the network's form).
CASES = [('aff 32->64 8x32 n1 plain', 1, 32, 64, 8, 32, L.PRO_NONE, 'plain', False),
         ('aff 64->96 16x64 n3 amax', 3, 64, 96, 16, 64, L.PRO_NONE, 'amax', False),
         ('relu 64->64 8x32 n3 stats', 3, 64, 64, 8, 32, L.PRO_RELU, 'stats', False),
         ('relu 32->96 16x64 n1 bias+res', 1, 32, 96, 16, 64, L.PRO_RELU, 'bias+res', False),
         ('swish 32->96 8x32 n3 bias+res', 3, 32, 96, 8, 32, L.PRO_SWISH, 'bias+res', False),
         ('swish 64->64 16x64 n1 plain', 1, 64, 64, 16, 64, L.PRO_SWISH, 'plain', False),
         ('swish 64->96 16x64 n3 stats', 3, 64, 96, 16, 64, L.PRO_SWISH, 'stats', False),
         ('swish 32->64 16x64 n3 amax', 3, 32, 64, 16, 64, L.PRO_SWISH, 'amax', False),
         ('swish 64->64 up 8x16 n3 stats', 3, 64, 64, 8, 16, L.PRO_SWISH, 'stats', True)]
IDS = [c[0] for c in CASES]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def bound_of(c, d):
    """(reference with bias and residual, bound) of one case: test_x1_prologue_numerics_against_fp64's docstring."""
    absx = extra = torch.zeros_like(d['ref16'])
    if d['b'] is not None:
        extra = d['b'].double().view(1, -1, 1, 1) + d['res'].double()
        absx = d['b'].double().abs().view(1, -1, 1, 1) + d['res'].double().abs()
    return d['ref16'] + extra, 9 * c[2] * 2.0 ** -24 * d['sabs16'] + 2.0 ** -22 * (d['ref16'].abs() + absx) + d['ambig'], extra, absx


def in_scale(amax):
    """The power of two the kernels multiply an image by (keep_conv_common.h: x3_range_scale): amax * s in [2^14, 2^15)."""
    return 2.0 ** (14 - math.floor(math.log2(amax)))


def ulp16(v):
    """Spacing of the fp16 grid at |v| (fp64 tensor): 2^(e - 10) in the normal range, 2^-24 below 2^-14."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


_CACHE = {}


def case(c):
    """Tensors and the fp64 reference of one case, computed once and shared (read-only) by the tests below.

    Inputs spread over several binades (log-normal gains per (image, channel) and per pixel); the affine carries a NON-ZERO shift per
    channel; in_amax[n] is the largest |prologue result| of image n, so the range scales differ between the images."""
    if c[0] in _CACHE:
        return _CACHE[c[0]]
    name, N, Cin, Cout, H, W, pro, epi, up = c
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = op_input(f'x1p_{name}', (N, Cin, H, W)) * torch.exp(1.2 * torch.randn(N, Cin, 1, 1, generator=g)) * torch.exp(0.5 * torch.randn(N, 1, H, W, generator=g))
    x = x * torch.tensor([1.0, 7.0, 0.2])[:N].view(N, 1, 1, 1)                       # images of different magnitude
    w = op_input(f'x1pw_{name}', (Cout, Cin, 3, 3), 1.0 / (3.0 * Cin ** 0.5)) * torch.exp(0.7 * torch.randn(Cout, Cin, 1, 1, generator=g))
    sc = (0.5 + op_input(f'x1ps_{name}', (N, Cin)).abs()) * torch.where(op_input(f'x1pg_{name}', (N, Cin)) > 0, 1.0, -1.0)
    sh = op_input(f'x1ph_{name}', (N, Cin), 1.5) + 0.25
    b = op_input(f'x1pb_{name}', (Cout,), 0.1) if epi == 'bias+res' else None
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    res = op_input(f'x1pr_{name}', (N, Cout, Ho, Wo)) if epi == 'bias+res' else None
    # the prologue in fp64 on the fp32 tensors (v = x * scale + shift; activation), then what the kernel rounds: fp16(act * s_n)
    v = x.double() * sc.double().view(N, Cin, 1, 1) + sh.double().view(N, Cin, 1, 1)
    act = v if pro == L.PRO_NONE else (v.clamp_min(0.0) if pro == L.PRO_RELU else v * torch.sigmoid(v))
    amax = act.reshape(N, -1).abs().amax(1).float()
    sa = torch.tensor([in_scale(float(a)) for a in amax], dtype=torch.float64).view(N, 1, 1, 1)
    a16 = (act * sa).to(torch.float16).double() / sa                                 # ONE rounding (a power-of-two scale is exact)
    # The kernel evaluates the prologue in fp32: an fma (<= 1/2 ulp of v), and under the swish -v log2(e) (1/2 ulp of the argument t, i.e.
    # |t| 2^-24 ln 2 relative in 2^t, as much again through v itself: d(v sigmoid v) / dv), v_exp_f32 and v_rcp_f32 (1 ulp = 2^-23 each),
    # one add, one multiply -- relative error of the result <= (8 + 1.5 |t|) 2^-24 (swish) / 2^-24 (affine, ReLU), against the fp64 value.  Where that interval straddles a rounding boundary
    # of the fp16 grid the kernel may legitimately round to the other neighbour: one fp16 spacing on that operand (`amb`), carried as its
    # own term of the bound.  It is zero for all but ~(8 + 1.5 |t|) 2^-12 of the elements.
    t = (v * 1.4426950408889634).abs()
    rel = (8.0 + 1.5 * t) * 2.0 ** -24 if pro == L.PRO_SWISH else torch.full_like(v, 2.0 ** -24)
    s_act = act * sa
    u = ulp16(s_act)
    frac = (s_act.abs() / u) % 1.0                                                   # position between two fp16 neighbours (ties at 0.5)
    amb = torch.where((frac - 0.5).abs() * u <= rel * s_act.abs() + 2.0 ** -149, u, torch.zeros_like(u)) / sa
    wp = w.permute(0, 2, 3, 1).contiguous()
    sw = ops.x3_scale_for(float(wp.abs().max()))
    w16p = (wp.reshape(-1) * sw).to(torch.float16)
    w16 = (w16p.double() / sw).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)

    def conv64(a, ww):
        a = F.interpolate(a, scale_factor=2, mode='nearest') if up else a
        return F.conv2d(a, ww, None, padding=1)                                       # zero padding of the ACTIVATED tensor
    d = dict(x=x, w=w, wp=wp, wx1=w16p.view(torch.int16), sw=sw, sc=sc, sh=sh, b=b, res=res, amax=amax, Ho=Ho, Wo=Wo,
             ref16=conv64(a16, w16), sabs16=conv64(a16.abs(), w16.abs()), ambig=conv64(amb, w16.abs()),
             ref=conv64(act, w.double()), sabs=conv64(act.abs(), w.double().abs()), amb_share=float((amb > 0).double().mean()))
    _CACHE[c[0]] = d
    return d


def conv_x1(c, d, stats):
    """ops.conv passes x3_in_amax only to prologue-free calls; these tests give the kernel its range scale with the prologue, so they
    build the argument struct themselves (the C-ABI is the interface under test)."""
    name, N, Cin, Cout, H, W, pro, epi, up = c
    Ho, Wo = d['Ho'], d['Wo']
    t = dict(x=nhwc(d['x']).cuda(), w=d['wp'].cuda(), wx1=d['wx1'].cuda(), sc=d['sc'].cuda().contiguous(), sh=d['sh'].cuda().contiguous(),
             amax=d['amax'].cuda(), out=torch.empty(N, Ho, Wo, Cout, device='cuda'))
    if d['b'] is not None:
        t['b'], t['res'] = d['b'].cuda(), nhwc(d['res']).cuda()
    a = L.conv_args(inp=t['x'], weight=t['w'], bias=t.get('b'), out=t['out'], pro_scale=t['sc'], pro_shift=t['sh'], residual=t.get('res'),
                    N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=Ho, Wo=Wo, in_ld=Cin, out_ld=Cout,
                    res_ld=Cout if 'res' in t else 0, upsample=int(up), pro_act=pro, mma=L.MMA_X1, weight_x3=t['wx1'], x3_acc_scale=1.0 / d['sw'],
                    x3_in_amax=t['amax'])
    pl = L.conv2d_plan(a)
    assert pl.kernel.decode() == X1_PRO_KERNEL[pro] and pl.split_k == 1 and pl.out_amax_ok, pl.kernel
    if stats == 'stats':
        t['part'] = torch.empty(N, pl.stats_P, Cout, 2, device='cuda')
        a.stats_out, a.stats_P = t['part'].data_ptr(), pl.stats_P
    if stats == 'amax':
        t['oamax'] = torch.zeros(N, device='cuda')
        a.x3_out_amax, a.x3_out_amax_zeroed = t['oamax'].data_ptr(), 1
    L.conv2d_launch(a)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_x1_prologue_numerics_against_fp64(c):
    """Reference: fp64 convolution of the ONCE-ROUNDED operands -- a16 = fp16(act(x scale + shift) s_n) / s_n with the prologue evaluated
    as the kernel orders it, w16 = fp16(w 2^e) 2^-e.  Against it only the fp32 accumulation and the epilogue's roundings remain, the
    accumulation part of tests/test_gpu_parsenet_f16.py::test_x1_kernel_numerics_against_fp64's bound:

        |err| <= K 2^-24 sum |a16 w16|  +  2^-22 (|ref| + |bias| + |residual|)  +  sum_{ambiguous k} ulp16(a_k) |w16_k|

    The last term is not an allowance for the kernel's arithmetic: it is the reference's own uncertainty about WHICH fp16 neighbour an
    activation rounds to when the fp32 evaluation of the prologue (hardware exp2 / rcp, 1 ulp each) lands within its error of a rounding
    boundary -- derived in case(); it vanishes for > 99 % of the elements.  Reported without assertion: the error against the UNROUNDED
    fp64 product and its ratio to that test's full bound (2^-10 + 2^-22 + K 2^-24) sum |a w|."""
    name, N, Cin, Cout, H, W, pro, epi, up = c
    d = case(c)
    t = conv_x1(c, d, epi)
    got = t['out'].permute(0, 3, 1, 2).cpu().double()
    K = 9 * Cin
    ref16, bound, extra, absx = bound_of(c, d)
    err = (got - ref16).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    full = (2.0 ** -10 + 2.0 ** -22 + K * 2.0 ** -24) * d['sabs'] + 2.0 ** -22 * (d['ref'].abs() + absx)
    e_un = (got - (d['ref'] + extra)).abs()
    print(f'[x1-prologue] {name} ({PRO_NAME[pro]}, {epi}): vs once-rounded fp64 max err {float(err.max()):.3e}, worst err / bound {ratio:.3f} '
          f'(ambiguous operands {d["amb_share"]:.2e}, their share of the bound at the worst point {float((d["ambig"] / bound)[err / bound == (err / bound).max()].max()):.2f}); '
          f'vs unrounded fp64 max err {float(e_un.max()):.3e}, worst ratio to the full 2^-10 bound {float((e_un / full).max()):.3f}; |ref| max {float(d["ref"].abs().max()):.3g}')
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (name, ratio)
    assert float((e_un / full).max()) > 2.0 ** -8          # really single fp16: an x3-grade result would sit near 2^-12 of that bound
    if epi == 'amax':
        assert torch.equal(t['oamax'].cpu(), t['out'].reshape(N, -1).abs().amax(1).cpu())


@pytest.mark.parametrize("c", [CASES[0], CASES[3], CASES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_zero_padding_is_applied_after_the_prologue(c):
    """The shift of every channel is non-zero (|shift| up to 1.75), so a prologue applied to padding pixels would put act(shift) where
    the reference has zeros: the border outputs then miss the bound by orders of magnitude, while they meet it as they are."""
    name, N, Cin, Cout, H, W, pro, epi, up = c
    d = case(c)
    got = conv_x1(c, d, 'plain')['out'].permute(0, 3, 1, 2).cpu().double()
    border = torch.ones(H, W, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    ref16, bound, _, _ = bound_of(c, d)
    err = (got - ref16).abs()
    assert float((err / bound)[:, :, border].max()) <= 1.0
    # what a padded-then-activated tensor would give: the difference at the border dwarfs the bound (the test can fail)
    v0 = d['sh'].double().view(N, Cin, 1, 1).expand(N, Cin, H + 2, W + 2).clone()
    act0 = v0 if pro == L.PRO_NONE else (v0.clamp_min(0.0) if pro == L.PRO_RELU else v0 * torch.sigmoid(v0))
    act0[:, :, 1:-1, 1:-1] = 0.0
    wrong = F.conv2d(act0, d['w'].double(), None)
    assert float((wrong.abs() / bound)[:, :, border].median()) > 100.0


@pytest.mark.parametrize("c", [CASES[2], CASES[6], CASES[8]], ids=[IDS[2], IDS[6], IDS[8]])
def test_groupnorm_partials_are_the_sums_of_the_kernels_own_output(c):
    """One (sum, sum of squares) partial per 256-pixel tile and channel: each equals the fp64 sum over the tile of the output the kernel
    wrote, within the fp32 summation error of 256 terms; and GroupNorm's scale / shift from them meet the standalone statistics kernels
    within the x3 statistics tests' 1e-5 (tests/test_gpu_kernels.py::test_conv_epilogue_stats_match_standalone)."""
    name, N, Cin, Cout, H, W, pro, epi, up = c
    d = case(c)
    t = conv_x1(c, d, 'stats')
    y = t['out']
    Ho, Wo = d['Ho'], d['Wo']
    tiles = y.double().view(N, Ho // 8, 8, Wo // 32, 32, Cout).permute(0, 1, 3, 5, 2, 4).reshape(N, -1, Cout, 256)
    part = t['part'].double()
    assert part.shape[1] == tiles.shape[1]
    for q, (s, sa) in enumerate(((tiles.sum(-1), tiles.abs().sum(-1)), ((tiles * tiles).sum(-1), (tiles * tiles).sum(-1)))):
        assert float(((part[..., q] - s).abs() / (257 * 2.0 ** -24 * sa + 1e-30)).max()) <= 1.0, (name, q)
    gamma, beta = op_input('x1p_gamma', (Cout,)).cuda() * 0.2 + 1, op_input('x1p_beta', (Cout,)).cuda() * 0.2
    st = ops.Stats(part=t['part'], P=t['part'].shape[1])
    sc, sh = ops.norm_affine(y, gamma, beta, 32, 1e-6, stats=st)
    sc2, sh2 = ops.norm_affine(y, gamma, beta, 32, 1e-6)
    for a_, b_, what in ((sc, sc2, 'scale'), (sh, sh2, 'shift')):
        assert float((a_ - b_).abs().max()) <= 1e-5 * max(1.0, float(b_.abs().max())), (name, what)


@pytest.mark.parametrize("c", [CASES[4], CASES[6], CASES[8]], ids=[IDS[4], IDS[6], IDS[8]])
def test_x1_prologue_memory_footprint(c):
    """Output, statistics and max|out| in poisoned surroundings (tests/footprint.py, the pattern of test_x1_kernel_memory_footprint):
    nothing outside them changes and no result depends on memory outside the inputs' payloads."""
    name, N, Cin, Cout, H, W, pro, epi, up = c
    d = case(c)
    Ho, Wo = d['Ho'], d['Wo']
    P = (Ho // 8) * (Wo // 32)
    res = d['res'] if d['res'] is not None else op_input(f'x1pfr_{name}', (N, Cout, Ho, Wo))
    b = d['b'] if d['b'] is not None else op_input(f'x1pfb_{name}', (Cout,), 0.1)
    tile = 4 * 340 * Cin * 4
    regions = [FP.single('x', nhwc(d['x']).reshape(-1, Cin), tile_bytes=tile), FP.single('w', d['wp'].reshape(Cout, -1)),
               FP.single('wx1', d['wx1'].view(torch.float16).reshape(Cout, -1)), FP.single('bias', b.reshape(1, -1)),
               FP.single('sc', d['sc'].reshape(N, Cin)), FP.single('sh', d['sh'].reshape(N, Cin)), FP.single('in_amax', d['amax'].reshape(1, -1)),
               FP.single('res', nhwc(res).reshape(-1, Cout), tile_bytes=256 * Cout * 4),
               FP.output('out', (N * Ho * Wo, Cout), tile_bytes=256 * Cout * 4), FP.output('part', (N * P, Cout * 2)), FP.output('amax', (1, N))]

    def run(t):
        a = L.conv_args(inp=t['x'], weight=t['w'], bias=t['bias'], out=t['out'], pro_scale=t['sc'], pro_shift=t['sh'], residual=t['res'], N=N, H=H, W=W,
                        Cin=Cin, Cout=Cout, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=Ho, Wo=Wo, in_ld=Cin, out_ld=Cout, res_ld=Cout, upsample=int(up),
                        pro_act=pro, mma=L.MMA_X1, weight_x3=t['wx1'], x3_acc_scale=1.0 / d['sw'], x3_in_amax=t['in_amax'], x3_out_amax=t['amax'],
                        stats_out=t['part'], stats_P=P)
        pl = L.conv2d_plan(a)
        assert pl.out_amax_ok and pl.split_k == 1 and pl.stats_P == P and pl.kernel.decode() == X1_PRO_KERNEL[pro], pl.kernel
        L.conv2d_launch(a)
        return pl.kernel.decode()
    out = FP.run(run, regions, 'cuda')
    assert torch.equal(out['amax'].reshape(N).cpu(), out['out'].reshape(N, -1).abs().amax(1).cpu())


def test_plan_names_the_x1_prologue_kernels_and_refuses_the_rest():
    ptr = torch.zeros(64, device='cuda')

    def plan(**kw):
        base = dict(N=2, H=16, W=64, Cin=64, Cout=64, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=16, Wo=64, in_ld=64, out_ld=64, mma=L.MMA_X1,
                    inp=ptr, out=ptr, weight=ptr, weight_x3=ptr, x3_acc_scale=1.0, pro_scale=ptr, pro_shift=ptr, pro_act=L.PRO_SWISH)
        base.update(kw)
        return L.conv2d_plan(L.conv_args(**base))
    for pro in (L.PRO_NONE, L.PRO_RELU, L.PRO_SWISH):
        pl = plan(pro_act=pro)
        assert pl.kernel.decode() == X1_PRO_KERNEL[pro] and pl.split_k == 1 and pl.out_amax_ok == 1 and pl.stats_P == 2 * 2
    assert plan(H=8, W=32, upsample=1).kernel.decode() == X1_PRO_KERNEL[L.PRO_SWISH]
    assert plan(pro_scale=None, pro_shift=None, pro_act=L.PRO_NONE).kernel.decode() == 'conv3x3_halo_x3s_kernel<0, false, true>'
    for bad in (dict(aux=ptr, residual=ptr, res_ld=64), dict(split_k=2), dict(Cin=48, in_ld=48), dict(flags=L.CONV_X3_EXACT_ACT),
                dict(H=12, W=20, Ho=12, Wo=20), dict(pad_mode=L.PAD_REFLECT)):      # (a prologue under reflection padding: refused as in v22)
        with pytest.raises(L.KeepHipError, match=r'code -2.*KEEP_MMA_X1 has no kernel'):
            plan(**bad)
    assert plan(flags=L.CONV_X3_EXACT_ACT, pro_act=L.PRO_RELU).kernel.decode() == X1_PRO_KERNEL[L.PRO_RELU]      # (only the swish has a fast form)
