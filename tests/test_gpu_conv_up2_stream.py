"""GPU suite (-m gpu): the streaming form of the x2-phase Upsample convolution (keep_conv_x3s.hip: conv3x3_up2_x3s_kernel -- two phases per
staged halo) against the stage-barrier form it replaces (conv3x3_halo_x3_kernel's UP2 instantiation, ``flags = CONV_NO_STREAM``).  Every
accumulator receives its products in the same order in both kernels and the epilogues add in the same order, so the outputs, the
GroupNorm partials and max|out| must be the same BITS; the fp64 judgement of the form is tests/test_gpu_kernels.py's
(test_conv_x3_upsample_as_four_phase_convolutions, test_conv_x3_at_the_shapes_of_the_step) and the case tables'."""
import pytest
import torch

from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops

pytestmark = pytest.mark.gpu

KERNEL = 'conv3x3_halo_x3_kernel<32, x2 phases>'

# The smallest shapes at which this pipeline can still go wrong (N, H, W, Cin, Cout, variant):
CASES = {
    # one tile holds all four borders; two chunks is the minimum; one cout block
    'one_tile': (1, 8, 32, 32, 64, 'plain'),
    # strided input (in_ld > Cin with an offset) and output (out_ld = 80, out_off = 12); the odd chunk count flips the halo-buffer parity
    # from item to item
    'strided_odd_chunks': (3, 8, 32, 48, 64, 'strided'),
    # residual = the output buffer itself; three cout blocks; interior tile edges in both directions
    'in_place_residual': (1, 16, 64, 32, 192, 'in_place'),
    # 640 items on at most 512 blocks: some blocks cross an item seam and an image boundary (the per-image max|out| bookkeeping)
    'item_seams': (5, 64, 64, 32, 256, 'plain'),
    # the other epilogue instantiation: no statistics, no residual
    'one_tile_no_stats': (1, 8, 32, 32, 64, 'no_stats'),
}
IN_LD_EXTRA, IN_OFF, OUT_LD, OUT_OFF = 8, 4, 80, 12


def run(case, flags):
    N, H, W, Cin, Cout, variant = CASES[case]
    tag = f'up2s_{N}_{H}_{W}_{Cin}_{Cout}'
    x = op_input(tag + '_x', (N, H, W, Cin), 2.0) + 0.3
    x[N - 1] *= 8.0                                        # per-image range scales differ
    w = op_input(tag + '_w', (Cout, 3, 3, Cin), 0.05)
    b = op_input(tag + '_b', (Cout,))
    w4 = ops.up2_phase_weights(w.cuda())
    sc4 = ops.x3_scale_for(float(w4.abs().max()))
    kw = dict(upsample=L.UPSAMPLE_X2_PHASES, wx3=ops.split_x3(w4.reshape(-1, Cin), sc4).view(-1), x3_acc_scale=1.0 / sc4, mma=L.MMA_X3,
              stats=variant != 'no_stats')
    xd = x.cuda()
    if variant == 'strided':
        wide = torch.full((N, H, W, Cin + IN_LD_EXTRA), 7.0, device='cuda')
        wide[..., IN_OFF:IN_OFF + Cin] = xd
        big = torch.zeros((N * 2 * H * 2 * W * OUT_LD + OUT_OFF,), device='cuda')
        kw.update(cin=Cin, in_off=IN_OFF, out=big[OUT_OFF:], out_ld=OUT_LD)
        xd = wide
    elif variant == 'in_place':
        buf = op_input(tag + '_r', (N, 2 * H, 2 * W, Cout)).cuda()
        kw.update(residual=buf, out=buf)
    old_flags, ops.DEFAULT.flags = ops.DEFAULT.flags, flags
    ops.DEFAULT.profile = []
    try:
        r = ops.conv(xd, w.cuda(), b.cuda(), **kw)
        name = ops.DEFAULT.profile[-1][0]
    finally:
        ops.DEFAULT.flags, ops.DEFAULT.profile = old_flags, None
    y, st = r if kw['stats'] else (r, None)
    if variant == 'strided':
        y = big
    torch.cuda.synchronize()
    return name, y, st


@pytest.mark.parametrize('case', list(CASES))
def test_up2_stream_reproduces_the_stage_barrier_kernel_bit_for_bit(case):
    """As planned (the streaming phase kernel: Cin >= 32) and under CONV_NO_STREAM (conv3x3_halo_x3_kernel's UP2 form): equal outputs --
    the gap columns of a strided output included --, equal statistics partials, equal max|out|."""
    name_s, y_s, st_s = run(case, 0)
    name_o, y_o, st_o = run(case, L.CONV_NO_STREAM)
    assert name_s == name_o == KERNEL, (name_s, name_o)
    assert torch.isfinite(y_s).all()
    assert float(y_s.abs().max()) > 0.0
    assert torch.equal(y_s, y_o), f'{int((y_s != y_o).sum())} of {y_s.numel()} outputs differ, max |d| {float((y_s - y_o).abs().max()):.3e}'
    if st_s is None:
        assert st_o is None
        return
    # (the library offers GroupNorm partials only for a dense output, out_ld == Cout: the strided case carries max|out| alone)
    assert st_s.P == st_o.P and (st_s.part is None) == (st_o.part is None) == (CASES[case][5] == 'strided')
    if st_s.part is not None:
        assert st_s.P == 4 * (CASES[case][1] // 8) * (CASES[case][2] // 32)      # one partial per (source tile, phase)
        assert torch.equal(st_s.part, st_o.part), f'{int((st_s.part != st_o.part).sum())} statistics partials differ'
    assert st_s.amax is not None and torch.equal(st_s.amax, st_o.amax)
    if CASES[case][5] == 'plain':      # (a strided / in-place output holds more than the convolution's values)
        assert torch.equal(st_s.amax.cpu(), y_s.abs().flatten(1).max(1).values.cpu())


def test_up2_plan_keeps_its_kernel_name():
    """The plan reports the family under the name bench.py and the step tests key on, also where the launch takes the streaming form."""
    x = op_input('up2s_name_x', (1, 8, 32, 128))
    w = op_input('up2s_name_w', (64, 3, 3, 128), 0.05)
    w4 = ops.up2_phase_weights(w.cuda())
    sc4 = ops.x3_scale_for(float(w4.abs().max()))
    ops.DEFAULT.profile = []
    try:
        ops.conv(x.cuda(), w.cuda(), None, upsample=L.UPSAMPLE_X2_PHASES, wx3=ops.split_x3(w4.reshape(-1, 128), sc4).view(-1),
                 x3_acc_scale=1.0 / sc4, mma=L.MMA_X3)
        name = ops.DEFAULT.profile[-1][0]
    finally:
        ops.DEFAULT.profile = None
    assert name == KERNEL, name
