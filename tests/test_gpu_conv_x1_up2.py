"""GPU suite (-m gpu): the single-fp16 form of the x2-phase Upsample convolution (KEEP_MMA_X1 with KEEP_CONV_X1_UP2: conv3x3_up2_x1s_kernel,
csrc/keep_conv_up2s.inc compiled with XU_X1 = true) -- numerics against fp64 from once-rounded operands, the statistics partials and max|out|,
the memory footprint under poisoned surroundings, batch invariance and the library's plan."""
import math

import pytest
import torch

import footprint as FP
from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu

# The smallest shapes at which this pipeline can still go wrong (N, H, W, Cin, Cout, variant):
CASES = {
    # one tile holds all four borders; one weight row serves both chunks of the item; one cout block
    'one_tile': (1, 8, 32, 32, 64, 'plain'),
    # strided input (in_ld > Cin with an offset) and output (out_ld = 80, out_off = 12); three 32-channel groups: an odd count of LDS-DMA rounds
    'strided_odd_groups': (3, 8, 32, 96, 64, 'strided'),
    # residual = the output buffer itself; three cout blocks; interior tile edges in both directions
    'in_place_residual': (1, 16, 64, 32, 192, 'in_place'),
    # 640 items on at most 512 blocks: some blocks cross an item seam and an image boundary (the per-image max|out| bookkeeping)
    'item_seams': (5, 64, 64, 32, 256, 'plain'),
    # the other epilogue instantiation (no statistics, no residual); two weight rows per item
    'one_tile_no_stats': (1, 8, 32, 64, 64, 'no_stats'),
}
IN_LD_EXTRA, IN_OFF, OUT_LD, OUT_OFF = 8, 4, 80, 12


def in_scale(amax):
    """The power of two the kernels multiply an image by (keep_conv_common.h: x3_range_scale): amax * s in [2^14, 2^15)."""
    return 2.0 ** (14 - math.floor(math.log2(amax)))


def phase_conv64(a, w4):
    """fp64 on the device: a [N,H,W,Cin], w4 [4,Cout,3,3,Cin] (``ops.up2_phase_weights``: phase py * 2 + px, taps on the source grid) ->
    [N,2H,2W,Cout], out[n, 2y+py, 2x+px] = sum over the 3 x 3 window centred on source pixel (y, x), zero padding."""
    N, H, W, Cin = a.shape
    Cout = w4.shape[1]
    ap = torch.zeros(N, H + 2, W + 2, Cin, dtype=torch.float64, device=a.device)
    ap[:, 1:-1, 1:-1] = a
    out = torch.zeros(N, 2 * H, 2 * W, Cout, dtype=torch.float64, device=a.device)
    for p in range(4):
        acc = torch.zeros(N, H, W, Cout, dtype=torch.float64, device=a.device)
        for kh in range(3):
            for kw in range(3):
                wt = w4[p, :, kh, kw, :]
                if bool((wt != 0).any()):
                    acc += ap[:, kh:kh + H, kw:kw + W].reshape(-1, Cin).matmul(wt.t()).view(N, H, W, Cout)
        out[:, p // 2::2, p % 2::2] = acc
    return out


_CACHE = {}


def case(name):
    """Tensors and the fp64 references of one case, computed once and shared (read-only) by the tests below.  The last image has 8 x the
    magnitude of the others, so the per-image range scales differ."""
    if name in _CACHE:
        return _CACHE[name]
    N, H, W, Cin, Cout, variant = CASES[name]
    tag = f'up2x1_{N}_{H}_{W}_{Cin}_{Cout}'
    x = op_input(tag + '_x', (N, H, W, Cin), 2.0) + 0.3
    x[N - 1] *= 8.0
    w = op_input(tag + '_w', (Cout, 3, 3, Cin), 0.05)
    b = op_input(tag + '_b', (Cout,))
    res = op_input(tag + '_r', (N, 2 * H, 2 * W, Cout)) if variant == 'in_place' else None
    amax = x.reshape(N, -1).abs().amax(1)
    w4 = ops.up2_phase_weights(w)
    sw = ops.x3_scale_for(float(w4.abs().max()))
    w16h = (w4 * sw).to(torch.float16)
    sa = torch.tensor([in_scale(float(a)) for a in amax], dtype=torch.float64).view(N, 1, 1, 1)
    xd, w4d = x.double().cuda(), w4.double().cuda()
    a16 = ((x.double() * sa).to(torch.float16).double() / sa).cuda()                # ONE rounding (a power-of-two scale is exact)
    w16 = (w16h.double() / sw).cuda()
    d = dict(x=x, w=w, b=b, res=res, amax=amax, sw=sw, wx1=w16h.view(torch.int16).reshape(-1),
             wx3=ops.split_x3(w4.reshape(-1, Cin), sw).view(-1),
             ref16=phase_conv64(a16, w16), sabs16=phase_conv64(a16.abs(), w16.abs()), ref=phase_conv64(xd, w4d), sabs=phase_conv64(xd.abs(), w4d.abs()))
    _CACHE[name] = d
    return d


def launch(name, d, mma, *, stats=True, images=None):
    """One keep_conv2d call of the case through the C-ABI (the interface under test).  mma: L.MMA_X1 (the bit and the hi-only phase twin) or
    L.MMA_X3 (the split phase twin).  ``images``: run only these images (a slice).  Returns the tensors of the call."""
    N, H, W, Cin, Cout, variant = CASES[name]
    sl = slice(0, N) if images is None else images
    x, amax = d['x'][sl].cuda(), d['amax'][sl].cuda().contiguous()
    n = x.shape[0]
    t = dict(w=d['w'].cuda(), b=d['b'].cuda(), amax=amax, wx=(d['wx1'] if mma == L.MMA_X1 else d['wx3']).cuda())
    in_ld, out_ld, inp = Cin, Cout, x
    if variant == 'strided':
        wide = torch.full((n, H, W, Cin + IN_LD_EXTRA), 7.0, device='cuda')
        wide[..., IN_OFF:IN_OFF + Cin] = x
        t['wide'], inp, in_ld = wide, wide.view(-1)[IN_OFF:], Cin + IN_LD_EXTRA
        t['big'] = torch.full((n * 2 * H * 2 * W * OUT_LD + OUT_OFF,), -3.0, device='cuda')
        t['out'], out_ld = t['big'][OUT_OFF:], OUT_LD
    elif variant == 'in_place':
        t['out'] = d['res'][sl].cuda().clone()
    else:
        t['out'] = torch.empty(n, 2 * H, 2 * W, Cout, device='cuda')
    a = L.conv_args(inp=inp, weight=t['w'], bias=t['b'], out=t['out'], residual=t['out'] if variant == 'in_place' else None,
                    N=n, H=H, W=W, Cin=Cin, Cout=Cout, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=2 * H, Wo=2 * W, in_ld=in_ld, out_ld=out_ld,
                    res_ld=Cout if variant == 'in_place' else 0, upsample=L.UPSAMPLE_X2_PHASES, mma=mma, weight_x3=t['wx'],
                    x3_acc_scale=1.0 / d['sw'], x3_in_amax=t['amax'], flags=L.CONV_X1_UP2 if mma == L.MMA_X1 else 0)
    pl = L.conv2d_plan(a)
    assert pl.kernel.decode() == (ops.X1_UP2_KERNEL if mma == L.MMA_X1 else 'conv3x3_halo_x3_kernel<32, x2 phases>'), pl.kernel
    assert pl.split_k == 1 and pl.out_amax_ok == 1
    if stats and variant != 'no_stats':
        if variant != 'strided':      # (the library offers GroupNorm partials only for a dense output: the strided case carries max|out| alone)
            assert pl.stats_P == 4 * (H // 8) * (W // 32)
            t['part'] = torch.empty(n, pl.stats_P, Cout, 2, device='cuda')
            a.stats_out, a.stats_P = t['part'].data_ptr(), pl.stats_P
        else:
            assert pl.stats_P == 0
        t['oamax'] = torch.zeros(n, device='cuda')
        a.x3_out_amax, a.x3_out_amax_zeroed = t['oamax'].data_ptr(), 1
    L.conv2d_launch(a)
    torch.cuda.synchronize()
    return t


def dense(name, t, n):
    """The convolution's values [n, 2H, 2W, Cout] of a call's output buffer."""
    N, H, W, Cin, Cout, variant = CASES[name]
    if variant == 'strided':
        return t['out'][:n * 4 * H * W * OUT_LD].view(n, 2 * H, 2 * W, OUT_LD)[..., :Cout]
    return t['out']


@pytest.mark.parametrize('name', list(CASES))
def test_x1_up2_numerics_against_fp64(name):
    """Reference: the fp64 phase convolution of the ONCE-ROUNDED operands, a16 = fp16(x s_n) / s_n with s_n the kernel's power of two for
    in_amax[n], w16 = fp16(w4 2^e) / 2^e with w4 = up2_phase_weights(w).  Against it only the fp32 accumulation of exact fp16 products and
    the epilogue's roundings remain (tests/test_gpu_conv_x1_prologue.py: bound_of, with the phase's four taps for its nine):

        |got - ref16| <= 4 Cin 2^-24 sum |a16 w16|  +  2^-22 (|ref16| + |bias| + |residual|)

    Against the UNROUNDED fp64 result the error must exceed the x3 form's on the same case: the launch really is single fp16."""
    N, H, W, Cin, Cout, variant = CASES[name]
    d = case(name)
    t = launch(name, d, L.MMA_X1)
    got = dense(name, t, N).double()
    extra = d['b'].double().cuda().view(1, 1, 1, -1).expand_as(got)
    absx = d['b'].double().abs().cuda().view(1, 1, 1, -1).expand_as(got)
    if variant == 'in_place':
        extra, absx = extra + d['res'].double().cuda(), absx + d['res'].double().abs().cuda()
    bound = 4 * Cin * 2.0 ** -24 * d['sabs16'] + 2.0 ** -22 * (d['ref16'].abs() + absx)
    err = (got - (d['ref16'] + extra)).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    e_x1 = float((got - (d['ref'] + extra)).abs().max())
    got3 = dense(name, launch(name, d, L.MMA_X3), N).double()
    e_x3 = float((got3 - (d['ref'] + extra)).abs().max())
    print(f'[x1-up2] {name}: vs once-rounded fp64 max err {float(err.max()):.3e}, worst err / bound {ratio:.3f}; vs unrounded fp64 max err '
          f'x1 {e_x1:.3e}, x3 {e_x3:.3e} (x1 / x3 = {e_x1 / max(e_x3, 1e-300):.1f}); |ref| max {float(d["ref"].abs().max()):.3g}')
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (name, ratio)
    assert e_x1 > e_x3, (name, e_x1, e_x3)
    if variant == 'strided':      # the gap columns of the strided output and the words in front of it are untouched
        assert bool((t['big'][:OUT_OFF] == -3.0).all())
        assert bool((t['out'][:N * 4 * H * W * OUT_LD].view(-1, OUT_LD)[:-1, Cout:] == -3.0).all())
    if variant == 'plain':        # max|out| of a dense output, exactly
        assert torch.equal(t['oamax'].cpu(), t['out'].reshape(N, -1).abs().amax(1).cpu())
    elif variant in ('strided', 'in_place'):      # (a strided buffer holds more than the convolution's values; in place the output is dense)
        assert torch.equal(t['oamax'].cpu(), dense(name, t, N).reshape(N, -1).abs().amax(1).cpu())


@pytest.mark.parametrize('name', ['one_tile', 'in_place_residual', 'item_seams'])
def test_partials_are_the_sums_of_the_kernels_own_output(name):
    """One (sum, sum of squares) partial per (8 x 32 source tile, phase) and channel: each equals the fp64 sum over that phase of the tile of
    the output the kernel wrote, within the fp32 summation error of 256 terms; and GroupNorm's scale / shift from them meet the standalone
    statistics kernels within the x3 statistics tests' 1e-5 (tests/test_gpu_conv_x1_prologue.py judges its partials the same way)."""
    N, H, W, Cin, Cout, variant = CASES[name]
    d = case(name)
    t = launch(name, d, L.MMA_X1)
    y = t['out']
    # [n, ty, r, py, tx, c, px, co] -> partial (ty * tiles_x + tx) * 4 + py * 2 + px
    tiles = y.double().view(N, H // 8, 8, 2, W // 32, 32, 2, Cout).permute(0, 1, 4, 3, 6, 7, 2, 5).reshape(N, -1, Cout, 256)
    part = t['part'].double()
    assert part.shape[1] == tiles.shape[1] == 4 * (H // 8) * (W // 32)
    for q, (s, sa) in enumerate(((tiles.sum(-1), tiles.abs().sum(-1)), ((tiles * tiles).sum(-1), (tiles * tiles).sum(-1)))):
        assert float(((part[..., q] - s).abs() / (257 * 2.0 ** -24 * sa + 1e-30)).max()) <= 1.0, (name, q)
    gamma, beta = op_input('up2x1_gamma', (Cout,)).cuda() * 0.2 + 1, op_input('up2x1_beta', (Cout,)).cuda() * 0.2
    st = ops.Stats(part=t['part'], P=t['part'].shape[1])
    sc, sh = ops.norm_affine(y, gamma, beta, 32, 1e-6, stats=st)
    sc2, sh2 = ops.norm_affine(y, gamma, beta, 32, 1e-6)
    for a_, b_, what in ((sc, sc2, 'scale'), (sh, sh2, 'shift')):
        assert float((a_ - b_).abs().max()) <= 1e-5 * max(1.0, float(b_.abs().max())), (name, what)
    if variant == 'plain':
        assert torch.equal(t['oamax'].cpu(), y.reshape(N, -1).abs().amax(1).cpu())


def test_a_batch_equals_its_images_run_alone():
    """Items are (image, source tile, row parity, cout block) and every accumulator takes its products in a fixed order: an N = 3 launch
    equals three N = 1 launches bit for bit, whatever the item-to-block assignment."""
    name = 'strided_odd_groups'
    N, H, W, Cin, Cout, _ = CASES[name]
    d = case(name)
    whole = launch(name, d, L.MMA_X1)
    for n in range(N):
        one = launch(name, d, L.MMA_X1, images=slice(n, n + 1))
        assert torch.equal(dense(name, one, 1), dense(name, whole, N)[n:n + 1]), n
        assert torch.equal(one['oamax'], whole['oamax'][n:n + 1]), n
    name = 'item_seams'
    N = CASES[name][0]
    d = case(name)
    whole = launch(name, d, L.MMA_X1)
    for n in (0, N - 1):
        one = launch(name, d, L.MMA_X1, images=slice(n, n + 1))
        assert torch.equal(one['out'], whole['out'][n:n + 1]) and torch.equal(one['part'], whole['part'][n:n + 1]), n


@pytest.mark.parametrize('name', ['one_tile', 'strided_odd_groups', 'in_place_residual'])
def test_x1_up2_memory_footprint(name):
    """Output, statistics and max|out| in poisoned surroundings (tests/footprint.py): nothing outside them changes -- the gap columns of the
    strided output included -- and no result depends on memory outside the inputs' payloads."""
    N, H, W, Cin, Cout, variant = CASES[name]
    d = case(name)
    Ho, Wo = 2 * H, 2 * W
    P = 4 * (H // 8) * (W // 32)
    strided, in_place = variant == 'strided', variant == 'in_place'
    tile = 4 * 340 * Cin * 4
    regions = [FP.single('x', d['x'].reshape(-1, Cin), ld=Cin + IN_LD_EXTRA if strided else None, off=IN_OFF if strided else 0, tile_bytes=tile),
               FP.single('w', d['w'].reshape(Cout, -1)), FP.single('wx1', d['wx1'].view(torch.float16).reshape(4 * Cout, -1)),
               FP.single('bias', d['b'].reshape(1, -1)), FP.single('in_amax', d['amax'].reshape(1, -1)), FP.output('amax', (1, N))]
    if in_place:
        regions.append(FP.single('out', d['res'].reshape(-1, Cout), role='rw', tile_bytes=256 * Cout * 4))
    else:
        regions.append(FP.output('out', (N * Ho * Wo, Cout), ld=OUT_LD if strided else None, off=OUT_OFF if strided else 0, tile_bytes=256 * Cout * 4))
    if not strided:
        regions.append(FP.output('part', (N * P, Cout * 2)))

    def run(t):
        a = L.conv_args(inp=t['x'], weight=t['w'], bias=t['bias'], out=t['out'], residual=t['out'] if in_place else None, N=N, H=H, W=W, Cin=Cin,
                        Cout=Cout, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=Ho, Wo=Wo, in_ld=t['x'].stride(0), out_ld=t['out'].stride(0),
                        res_ld=t['out'].stride(0) if in_place else 0, upsample=L.UPSAMPLE_X2_PHASES, mma=L.MMA_X1, weight_x3=t['wx1'],
                        x3_acc_scale=1.0 / d['sw'], x3_in_amax=t['in_amax'], x3_out_amax=t['amax'], flags=L.CONV_X1_UP2,
                        stats_out=None if strided else t['part'], stats_P=0 if strided else P)
        pl = L.conv2d_plan(a)
        assert pl.out_amax_ok and pl.split_k == 1 and pl.stats_P == (0 if strided else P) and pl.kernel.decode() == ops.X1_UP2_KERNEL, pl.kernel
        L.conv2d_launch(a)
        return pl.kernel.decode()
    out = FP.run(run, regions, 'cuda')
    assert torch.equal(out['amax'].reshape(N).cpu(), out['out'].reshape(N, -1).abs().amax(1).cpu())


def test_ops_routes_the_up2_branch_to_the_planned_kernel():
    """``Ops.up2_x1``: conv(upsample=True) of an x3 Ops runs the new kernel string where the library admits it (and only there), with the same
    values as the C-ABI call above; off, it launches x3's."""
    name = 'one_tile'
    N, H, W, Cin, Cout, _ = CASES[name]
    d = case(name)
    o = ops.Ops()
    blob = d['w'].reshape(-1).cuda()
    bx3, table = ops.make_x3_blob(blob, {'w': (0, (Cout, 3, 3, Cin))}, {'w': blob.view(Cout, 3, 3, Cin)}, ['w'])
    o.set_precision(L.MMA_X3, blob, None, bx3, 1.0, x3_scales=table)
    w = blob.view(Cout, 3, 3, Cin)
    x = d['x'].cuda()
    seen = {}
    for knob in (False, True):
        o.up2_x1, o.census = knob, {}
        y, st = o.conv(x, w, d['b'].cuda(), upsample=True, stats=True)
        seen[knob] = (dict(o.census), y, st)
    assert seen[False][0] == {'conv3x3_halo_x3_kernel<32, x2 phases>': 1} and seen[True][0] == {ops.X1_UP2_KERNEL: 1}
    ref = launch(name, d, L.MMA_X1)
    assert torch.equal(seen[True][1], ref['out']) and torch.equal(seen[True][2].part, ref['part']) and torch.equal(seen[True][2].amax, ref['oamax'])
    assert not torch.equal(seen[False][1], seen[True][1])
    # a 16-channel input has no 32-channel groups: the library refuses, the call stays x3
    w16 = op_input('up2x1_w16', (64, 3, 3, 16), 0.05).reshape(-1).cuda()
    bx3, table = ops.make_x3_blob(w16, {'w': (0, (64, 3, 3, 16))}, {'w': w16.view(64, 3, 3, 16)}, ['w'])
    o.set_precision(L.MMA_X3, w16, None, bx3, 1.0, x3_scales=table)
    o.census = {}
    o.conv(op_input('up2x1_x16', (1, 8, 32, 16)).cuda(), w16.view(64, 3, 3, 16), None, upsample=True)
    assert o.census == {'conv3x3_halo_x3_kernel<32, x2 phases>': 1}
