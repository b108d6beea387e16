"""GPU suite (-m gpu): conv3x3_halo_x3s_kernel (keep_conv_x3s.hip, the streaming x3 3x3 convolution) after its schedule work -- item
constants recomputed at the item transitions instead of kept (spilled) across the MFMA loops, the epilogue activation a template argument.
The kernel's term order differs from the stage-barrier kernel's, so bit-equality is against ITSELF.  Per case:
  (i)   against fp64: every output within 2e-6 of its own sum |x| |w| (x: what enters the multiplication, i.e. behind the prologue) --
        tests/test_gpu_kernels.py's bound for x3 convolutions, taken per output;
  (ii)  output, statistics partials and max|out| of every image of the batched launch == those of the image launched alone, bit for bit;
  (iii) two runs of the same launch are bit-equal;
  (iv)  max|out| == the maximum of the written tensor, exactly.
The epilogue activation is a template argument of the kernel: the cases with one run conv3x3_halo_x3s_act_kernel<PRO, AFF, X1, EACT> -- ReLU, SiLU
(YOLOv5-face's) and LeakyReLU (ParseNet's 0.2 under reflection padding, RetinaFace's 0.1 behind a prologue) -- in the x3 and the single-fp16 (x1)
form.  The x1 cases keep (ii)-(iv) as they are; their bound in (i) comes from the format: both operands are rounded ONCE to fp16 (relative error
<= 2^-11 each, the range scale is a power of two), so a product is off by at most 2^-10 of |x| |w| to first order, plus the x3 bound for the fp32
accumulation and epilogue: (2^-10 + 2e-6) sum |x| |w| per output.
Every launch carries CONV_NO_SMALL_PARTIALS: without it launches of at most 64 items go to the 64-pixel-block kernels (same values, another
kernel), and these shapes are the smallest at which the streaming pipeline can still go wrong."""
import pytest
import torch
import torch.nn.functional as F

from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu

KERNEL = 'conv3x3_halo_x3s_kernel'                       # the plan's name of the x3 form (every prologue, every activation)
KERNEL_X1 = 'conv3x3_halo_x3s_kernel<0, false, true>'    # ... and of the single-fp16 form on raw inputs
ACTS = {'relu': (L.ACT_RELU, torch.relu), 'silu': (L.ACT_SILU, F.silu), 'lrelu01': (L.ACT_LRELU01, lambda t: F.leaky_relu(t, 0.1)),
        'lrelu02': (L.ACT_LRELU02, lambda t: F.leaky_relu(t, 0.2))}
IN_LD_EXTRA, IN_OFF, OUT_LD, OUT_OFF = 8, 4, 80, 12

# (N, H, W, Cin, Cout, prologue, variant[, epilogue activation[, 'x1']])
CASES = {
    # one tile holds all four borders; two chunks is the minimum; each prologue form is an instantiation of its own
    'raw': (1, 8, 32, 32, 64, 'raw', 'plain'),
    'affine': (1, 8, 32, 32, 64, 'affine', 'plain'),
    'affine_relu': (1, 8, 32, 32, 64, 'relu', 'plain'),
    'affine_swish': (1, 8, 32, 32, 64, 'swish', 'plain'),
    # x[2] *= 8: the per-image range scales differ; strided input and output; the odd chunk count flips the halo-buffer parity from item to item
    'strided_odd_chunks': (3, 8, 32, 48, 64, 'raw', 'strided'),
    # residual = the output buffer itself; three cout blocks; interior tile edges in both directions
    'in_place_residual': (1, 16, 64, 32, 192, 'swish', 'in_place'),
    # 576 items on at most 512 blocks: blocks cross item seams and image boundaries (the per-image max|out| bookkeeping)
    'item_seams': (9, 64, 64, 32, 256, 'swish', 'plain'),
    # no GroupNorm partials (the epilogue's other branch); max|out| alone
    'no_stats': (1, 8, 32, 32, 64, 'raw', 'no_stats'),
    # ParseNet's form: reflection padding, LeakyReLU(0.2) in the epilogue -- the activation instantiation
    'reflect_lrelu': (2, 16, 32, 32, 64, 'raw', 'reflect', 'lrelu02'),
    # the other activation instantiations the engines reach on raw inputs, and one behind a prologue
    'raw_relu': (1, 8, 32, 32, 64, 'raw', 'plain', 'relu'),
    'raw_silu': (2, 8, 32, 32, 64, 'raw', 'plain', 'silu'),
    'swish_lrelu01': (1, 8, 32, 32, 64, 'swish', 'plain', 'lrelu01'),
    # single fp16: the same pipeline with 36 MFMAs per chunk
    'x1_raw_silu': (2, 8, 32, 32, 64, 'raw', 'plain', 'silu', 'x1'),
    'x1_raw_relu': (1, 8, 32, 32, 64, 'raw', 'plain', 'relu', 'x1'),
    'x1_reflect_lrelu': (2, 16, 32, 32, 64, 'raw', 'reflect', 'lrelu02', 'x1'),
}


def case_of(case):
    c = CASES[case]
    return c[:7] + (c[7] if len(c) > 7 else None, len(c) > 8)


def inputs(case):
    N, H, W, Cin, Cout, pro, variant, act, x1 = case_of(case)
    tag = f'x3ss_{case}'
    x = op_input(tag + '_x', (N, H, W, Cin), 2.0) + 0.3
    if variant == 'strided':
        x[2] *= 8.0
    d = dict(x=x, w=op_input(tag + '_w', (Cout, 3, 3, Cin), 0.05), b=op_input(tag + '_b', (Cout,)))
    if pro != 'raw':
        d['sc'] = op_input(tag + '_ps', (N, Cin)) * 0.2 + 1.0
        d['sh'] = op_input(tag + '_ph', (N, Cin)) * 0.2
    if variant == 'in_place':
        d['res'] = op_input(tag + '_r', (N, H, W, Cout))
    return d


def launch(case, d, images):
    """One launch on the images ``images`` (a slice of the batch); (kernel name, written values [n, H, W, Cout], the whole written buffer, Stats)."""
    N, H, W, Cin, Cout, pro, variant, act, x1 = case_of(case)
    n = len(range(N)[images])
    wd = d['w'].cuda()
    sc = ops.x3_scale_for(float(wd.abs().max()))
    twin = (wd.reshape(-1) * sc).to(torch.float16).view(torch.int16) if x1 else ops.split_x3(wd.reshape(-1, Cin), sc).view(-1)
    kw = dict(mma=L.MMA_X1 if x1 else L.MMA_X3, wx3=twin, x3_acc_scale=1.0 / sc, stats='amax' if variant == 'no_stats' else True, split_k=1)
    xd = d['x'][images].cuda()
    if pro != 'raw':
        kw.update(pro=(d['sc'][images].cuda().contiguous(), d['sh'][images].cuda().contiguous()),
                  pro_act={'affine': L.PRO_NONE, 'relu': L.PRO_RELU, 'swish': L.PRO_SWISH}[pro])
    big = None
    if variant == 'strided':
        wide = torch.full((n, H, W, Cin + IN_LD_EXTRA), 7.0, device='cuda')
        wide[..., IN_OFF:IN_OFF + Cin] = xd
        big = torch.full((n * H * W * OUT_LD + OUT_OFF,), -3.0, device='cuda')
        kw.update(cin=Cin, in_off=IN_OFF, out=big[OUT_OFF:], out_ld=OUT_LD)
        xd = wide
    elif variant == 'in_place':
        buf = d['res'][images].cuda().contiguous()
        kw.update(residual=buf, out=buf)
    elif variant == 'reflect':
        kw.update(reflect=True)
    if act:
        kw.update(act=ACTS[act][0])
    old_flags, ops.DEFAULT.flags = ops.DEFAULT.flags, L.CONV_NO_SMALL_PARTIALS
    ops.DEFAULT.profile = []
    try:
        y, st = ops.conv(xd, wd, d['b'].cuda(), **kw)
        name = ops.DEFAULT.profile[-1][0]
    finally:
        ops.DEFAULT.flags, ops.DEFAULT.profile = old_flags, None
    torch.cuda.synchronize()
    whole = y
    if variant == 'strided':
        whole = big
        y = big[OUT_OFF:].view(n, H, W, OUT_LD)[..., :Cout]
    return name, y, whole, st


def reference(case, d):
    """fp64 on the GPU (unfold + matmul): the convolution's value and sum |x| |w| per output."""
    N, H, W, Cin, Cout, pro, variant, act, x1 = case_of(case)
    x = d['x'].cuda().double()
    if pro != 'raw':
        x = x * d['sc'].cuda().double().view(N, 1, 1, Cin) + d['sh'].cuda().double().view(N, 1, 1, Cin)
        x = {'affine': lambda t: t, 'relu': torch.relu, 'swish': lambda t: t * torch.sigmoid(t)}[pro](x)
    x = x.permute(0, 3, 1, 2)
    x = F.pad(x, (1, 1, 1, 1), mode='reflect') if variant == 'reflect' else F.pad(x, (1, 1, 1, 1))      # (zero padding follows the prologue)
    cols = F.unfold(x, 3)                                                       # [N, Cin * 9, H * W], rows ordered (channel, kh, kw)
    wm = d['w'].cuda().double().permute(0, 3, 1, 2).reshape(Cout, Cin * 9)      # [Cout][kh][kw][Cin] -> (channel, kh, kw)
    ref = (wm @ cols).view(N, Cout, H, W).permute(0, 2, 3, 1) + d['b'].cuda().double()
    mag = (wm.abs() @ cols.abs()).view(N, Cout, H, W).permute(0, 2, 3, 1)
    if act:
        ref = ACTS[act][1](ref)
    if variant == 'in_place':
        ref = ref + d['res'].cuda().double()
    return ref, mag


@pytest.mark.parametrize('case', list(CASES))
def test_streaming_x3_conv(case):
    N, H, W, Cin, Cout, pro, variant, act, x1 = case_of(case)
    d = inputs(case)
    name, y, whole, st = launch(case, d, slice(0, N))
    assert name == (KERNEL_X1 if x1 else KERNEL), name
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0.0
    # (i) fp64
    ref, mag = reference(case, d)
    err = (y.double() - ref).abs()
    ratio = float((err / mag).max())
    bound = 2.0 ** -10 + 2e-6 if x1 else 2e-6
    print(f'{case}: max err / sum|x||w| = {ratio:.3e} (bound {bound:.3e}), max err {float(err.max()):.3e}')
    assert bool((err <= bound * mag).all()), f'{int((err > bound * mag).sum())} of {err.numel()} outputs beyond {bound:.3e} sum|x||w|; worst ratio {ratio:.3e}'
    # (iii) run to run
    _, y2, whole2, st2 = launch(case, d, slice(0, N))
    assert torch.equal(whole, whole2), f'{int((whole != whole2).sum())} outputs differ between two runs'
    assert torch.equal(st.amax, st2.amax)
    dense = variant not in ('strided', 'no_stats')      # (GroupNorm partials come with a dense output, out_ld == Cout, and are not asked for under 'no_stats')
    assert (st.part is not None) == dense
    if dense:
        assert st.P == (H // 8) * (W // 32)             # one partial per 256-pixel tile
        assert torch.equal(st.part, st2.part)
    # (iv) max|out| of what was written
    assert torch.equal(st.amax.cpu(), y.abs().flatten(1).max(1).values.cpu())
    if variant == 'strided':                            # nothing outside the output windows was written
        assert bool((whole[:OUT_OFF] == -3.0).all())
        assert bool((whole[OUT_OFF:].view(-1, OUT_LD)[:, Cout:] == -3.0).all())
    # (ii) every image alone
    for n in range(N if N > 1 else 0):
        _, y1, _, st1 = launch(case, d, slice(n, n + 1))
        assert torch.equal(y1[0], y[n]), f'image {n}: {int((y1[0] != y[n]).sum())} outputs differ from the batched launch'
        assert torch.equal(st1.amax[0], st.amax[n]), f'image {n}: max|out| differs'
        if dense:
            assert torch.equal(st1.part[0], st.part[n]), f'image {n}: {int((st1.part[0] != st.part[n]).sum())} statistics partials differ'
