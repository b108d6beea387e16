"""GPU suite (-m gpu): ParseNet's opt-in single-fp16 precision ('f16', KEEP_MMA_X1) -- kernel numerics against fp64 with a derived
bound, memory footprint, the network against the reference logits of tests/golden/facelib.npz, batch invariance, the composite
and the untouched default path."""
import math
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import footprint as FP
from conftest import GOLDEN, op_input
from comfyui_keep_amd.engine import hiplib as L
from comfyui_keep_amd.engine import ops
from comfyui_keep_amd.engine import parsenet as PN

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(GOLDEN, 'facelib.npz'))

# max |logit_f16 - logit_reference| over the golden logit grids, MEASURED on an MI355X (2026-10-17): 1.25 x the figure, rounded up to
# two significant digits (the kernels are deterministic; the margin covers another plan choice at another batch size).  The x3
# policy's figure on the same grids is 1e-4 .. 3e-4 (logits of +-58 / +-115).  Measured: see E16_MEASURED.
E16_MEASURED = {'parsenet128': 6.9309e-02, 'parsenet512': 1.5336e-01}      # (x3 on the same grids: 1.2e-4 / 3.1e-4)
E16_BOUND = 0.20                     # 1.25 x 0.15336 = 0.1917 -> 0.20
# the composite: max uint8 difference / share of differing pixels of the 1080p 3-face paste between 'f16' and 'x3' class maps, as measured
PASTE_MAX_MEASURED, PASTE_SHARE_MEASURED = 1, 7.937e-3      # (the class maps differ in 1094 of 786432 pixels)

# (name, N, Cin, Cout, H, W, stride, upsample): one shape per ParseNet(512, 512) launch kind
KINDS = [('stride-1 3x3 64ch', 2, 64, 64, 32, 64, 1, False),
         ('stride-1 3x3 256ch 32^2', 1, 256, 256, 32, 32, 1, False),
         ('stride-2 3x3', 1, 64, 128, 128, 128, 2, False),      # (large enough for an un-split plan: the fused max|out| needs one)
         ('upsample then conv', 2, 128, 64, 16, 32, 1, True),
         ('3 -> 64 first', 2, 3, 64, 32, 32, 1, False),
         ('64 -> 19 padded to 32', 2, 64, 32, 32, 32, 1, False)]


X1_KERNELS = ('conv3x3_halo_x3s_kernel<0, false, true>', 'conv_x3_kernel<2, 2, 1, 1, true, 0, 0, 1, 0, 1>',
              'conv_x3_kernel<2, 2, 2, 2, true, 0, 0, 1, 0, 1>')      # the x1 instantiations, as keep_conv2d_plan names them


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def spread_input(name, shape):
    """Signed values with a realistic spread: uniform +-1 times a log-normal per-(image, channel) gain (sigma 1.2) and a per-pixel gain
    (sigma 0.5), so that sum |a w| is far from |sum a w| and a good share of the scaled operands sits well below the maximum."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    N, C, H, W = shape
    x = op_input(f'f16_{name}', shape)
    return x * torch.exp(1.2 * torch.randn(N, C, 1, 1, generator=g)) * torch.exp(0.5 * torch.randn(N, 1, H, W, generator=g))


def kind_tensors(kind):
    name, N, Cin, Cout, H, W, stride, up = kind
    x = spread_input(name, (N, Cin, H, W))
    w = op_input(f'f16w_{name}', (Cout, Cin, 3, 3), 1.0 / (3.0 * Cin ** 0.5))
    w = w * torch.exp(0.7 * torch.randn(Cout, Cin, 1, 1, generator=torch.Generator().manual_seed(11)))
    if Cout == 32 and 'padded' in name:
        w[19:] = 0.0                              # the 19 class maps padded to 32 output channels (engine/parsenet.py)
    b = op_input(f'f16b_{name}', (Cout,), 0.1)
    return x, w, b


def x1_twin(wp, Cin):
    sc = ops.x3_scale_for(float(wp.abs().max()))
    return (wp.reshape(-1) * sc).to(torch.float16).view(torch.int16), sc


def in_scale(amax):
    """The power of two the kernels multiply an image by (keep_conv_common.h: x3_range_scale): amax * s in [2^14, 2^15)."""
    return 2.0 ** (14 - math.floor(math.log2(amax)))


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_x1_kernel_numerics_against_fp64(kind):
    """Each operand is multiplied by an exact power of two and rounded once to fp16: inside the normal range <= 2^-11 relative each, so a
    product carries <= 2^-10 + 2^-22; the fp32 accumulation of K terms adds <= K 2^-24 of the running magnitude (<= sum |a w|):

        |err| <= (2^-10 + 2^-22 + K 2^-24) sum |a w|  +  floor  +  2^-22 (|ref| + |bias|)

    floor: a scaled operand below 2^-14 is rounded on the subnormal grid, absolute error <= 2^-25 in scaled units, i.e. 2^-25 / s_a per
    activation and 2^-25 / s_w per weight -> sum_k (|w_k| / s_a + |a_k| / s_w) 2^-25 (1 + 2^-10).  The last term: the fp32 roundings
    of the epilogue (accumulator scale is exact; the bias add and the store round once each).  sum |a w| and |ref| come from fp64."""
    name, N, Cin, Cout, H, W, stride, up = kind
    x, w, b = kind_tensors(kind)
    xin = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
    xp = F.pad(xin.double(), (1, 1, 1, 1), mode='reflect')
    ref = F.conv2d(xp, w.double(), b.double(), stride=stride)
    sabs = F.conv2d(xp.abs(), w.double().abs(), None, stride=stride)
    wp = w.permute(0, 2, 3, 1).contiguous().cuda()
    # (the 3 -> 64 layer has no x1 kernel: the engine runs it on its base policy, exact f32)
    kw = dict(stride=stride, pad=1, ksize=3, upsample=up, reflect=True, mma=L.MMA_X1 if Cin % 32 == 0 else L.MMA_F32, stats='amax')
    floor = torch.zeros_like(ref)
    if Cin % 32 == 0:
        tw, sw = x1_twin(wp, Cin)
        kw.update(wx3=tw, x3_acc_scale=1.0 / sw)
        sa = torch.tensor([in_scale(float(x[n].abs().max())) for n in range(N)], dtype=torch.float64).view(N, 1, 1, 1)
        ones = torch.ones_like(w, dtype=torch.float64)
        floor = (F.conv2d(torch.ones_like(xp), w.double().abs(), None, stride=stride) / sa
                 + F.conv2d(xp.abs(), ones, None, stride=stride) / sw) * 2.0 ** -25 * (1 + 2.0 ** -10)
    y, st = ops.conv(nhwc(x), wp, b.cuda(), **kw)
    torch.cuda.synchronize()
    got = y.permute(0, 3, 1, 2).cpu().double()
    K = 9 * Cin
    bound = (2.0 ** -10 + 2.0 ** -22 + K * 2.0 ** -24) * sabs + floor + 2.0 ** -22 * (ref.abs() + b.double().abs().view(1, -1, 1, 1))
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    print(f'[x1-numerics] {name}: max err {float(err.max()):.3e} (|ref| max {float(ref.abs().max()):.3g}), worst err / bound {ratio:.3f}, '
          f'|sum| / sum|.| median {float((ref - b.double().view(1, -1, 1, 1)).abs().div(sabs + 1e-300).median()):.3f}, floor share {float((floor / bound).max()):.2e}')
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, (name, ratio)
    if Cin % 32 == 0:                             # the fused max |out| of the epilogue: the next layer's range scale
        assert st is not None and torch.equal(st.amax.cpu(), y.reshape(N, -1).abs().amax(1).cpu())
        # the x1 kernel, not a quiet change of policy: away from x3's fp32-grade result by an fp16 rounding's worth
        y3 = ops.conv(nhwc(x), wp, b.cuda(), **dict(kw, mma=L.MMA_X3, stats=False, wx3=ops.split_x3(wp.reshape(-1, Cin), sw).view(-1)))
        assert float((y3 - y).abs().max()) > 2.0 ** -16 * float(sabs.max()) * 1e-2
    if 'padded' in name:
        assert not y[..., 19:].sub(b.cuda()[19:]).any()      # zero weight rows: bias only


@pytest.mark.parametrize("kind", [k for k in KINDS if k[2] % 32 == 0], ids=[k[0] for k in KINDS if k[2] % 32 == 0])
def test_x1_kernel_memory_footprint(kind):
    """The same launch kinds in poisoned surroundings (tests/footprint.py): nothing outside the declared output and max|out| slots
    changes, no result depends on memory outside the inputs' payloads.  Every buffer is the test's own."""
    name, N, Cin, Cout, H, W, stride, up = kind
    x, w, b = kind_tensors(kind)
    Hv, Wv = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hv - 1) // stride + 1, (Wv - 1) // stride + 1
    wp = w.permute(0, 2, 3, 1).contiguous()
    sw = ops.x3_scale_for(float(wp.abs().max()))
    tw = (wp.reshape(-1) * sw).to(torch.float16)
    amax = x.reshape(N, -1).abs().amax(1)
    res = op_input(f'f16r_{name}', (N * Ho * Wo, Cout))
    tile = 4 * 340 * Cin * 4
    regions = [FP.single('x', x.permute(0, 2, 3, 1).contiguous().reshape(-1, Cin), tile_bytes=tile),
               FP.single('w', wp.reshape(Cout, -1)), FP.single('wx1', tw.reshape(Cout, -1)), FP.single('bias', b.reshape(1, -1)),
               FP.single('in_amax', amax.reshape(1, -1)), FP.single('res', res, tile_bytes=256 * Cout * 4),
               FP.output('out', (N * Ho * Wo, Cout), tile_bytes=256 * Cout * 4), FP.output('amax', (1, N))]

    def launch(t):
        a = L.conv_args(inp=t['x'], weight=t['w'], bias=t['bias'], out=t['out'], residual=t['res'], N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=3, KW=3,
                        stride=stride, pad_t=1, pad_l=1, Ho=Ho, Wo=Wo, in_ld=Cin, out_ld=Cout, res_ld=Cout, upsample=int(up), epi_act=L.ACT_LRELU02,
                        mma=L.MMA_X1, weight_x3=t['wx1'], x3_acc_scale=1.0 / sw, x3_in_amax=t['in_amax'], x3_out_amax=t['amax'],
                        pad_mode=L.PAD_REFLECT)
        pl = L.conv2d_plan(a)
        assert pl.out_amax_ok and pl.split_k == 1 and pl.kernel.decode() in X1_KERNELS, pl.kernel
        L.conv2d_launch(a)
        return pl.kernel.decode()
    out = FP.run(launch, regions, 'cuda')
    assert torch.equal(out['amax'].reshape(N).cpu(), out['out'].reshape(N, -1).abs().amax(1).cpu())


def test_attention_refuses_x1():
    q = torch.zeros(1, 64, 64, device='cuda')
    with pytest.raises(L.KeepHipError, match='KEEP_MMA_X1'):
        ops.attention(q, q, q, torch.empty_like(q), B=1, H=1, Lq=64, Lk=64, D=64, Dv=64, scale=1.0, q_str=(4096, 64, 64), k_str=(4096, 64, 64),
                      v_str=(4096, 64, 64), o_str=(4096, 64, 64), mma=L.MMA_X1)


def _golden_fixture_share(key, thr):
    return float((G[f'{key}_margin'].astype(np.float32) > thr).mean())


def test_parsenet_f16_against_the_reference_logits():
    """ParseNetEngine(precision='f16') on the ParseNet inputs of the golden file (logit grids and classes from the reference module): the
    logit error stays inside E16_BOUND, and a pixel whose class differs from the reference arg-max has a reference top-1 / top-2 margin
    of at most 2 E16_BOUND (two logits move by at most E16_BOUND each)."""
    errs = {}
    for key, size, n, gy, gx, step in (('parsenet128', 128, 2, 1, 2, 4), ('parsenet512', 512, 1, 3, 5, 16)):
        W = PN.synth_parsenet_state_dict(seed=0, in_size=size, out_size=size)
        eng = PN.ParseNetEngine(W, in_size=size, out_size=size, precision='f16').to('cuda')
        assert eng.o.mma == L.MMA_F32 and eng.o.blobx1 is not None and eng.o.blobx3 is None      # the twin rides on exact f32
        x = op_input(key, (n, 3, size, size))
        logits = eng.logits(x.cuda()).cpu().numpy()
        assert np.isfinite(logits).all()
        grid = G[f'{key}_logit_grid']
        errs[key] = float(np.abs(logits[:, :, gy::step, gx::step] - grid).max())
        e3 = PN.ParseNetEngine(W, in_size=size, out_size=size, precision='x3').to('cuda')
        ex3 = float(np.abs(e3.logits(x.cuda()).cpu().numpy()[:, :, gy::step, gx::step] - grid).max())
        cls = eng.classes(nhwc(x)).cpu().numpy()
        margin = G[f'{key}_margin'].astype(np.float32)
        differs = cls != G[f'{key}_classes']
        worst = float(margin[differs].max()) if differs.any() else 0.0
        print(f'[f16-network] {key}: E16 {errs[key]:.4e} (x3 on the same grid {ex3:.3e}; logit scale {np.abs(grid).max():.1f}); '
              f'{int(differs.sum())} of {differs.size} pixels change class, largest reference margin among them {worst:.4e}')
        errs[key + '_worst_margin'] = worst
        assert errs[key] > 4 * ex3                # really the single-fp16 kernels
    assert E16_BOUND is not None, f'E16_BOUND not recorded yet; measured {errs}'
    for key in ('parsenet128', 'parsenet512'):
        assert errs[key] <= E16_BOUND, (key, errs[key])
        assert errs[key + '_worst_margin'] <= 2 * E16_BOUND, (key, errs[key + '_worst_margin'])
        # condition on the fixture (also checkable on the CPU from the golden alone): the pixels the statement above protects
        assert _golden_fixture_share(key, 2 * E16_BOUND) >= 0.90, (key, _golden_fixture_share(key, 2 * E16_BOUND))


# the kernel of the one layer without an x1 twin (the Cin = 3 convolution) under 'f16', as keep_conv2d_plan names it: read off the 'f16' launch
# list of ParseNetEngine(128, 128) at commit bc12ff0 (where 'f16' was an Ops policy of its own) -- exact f32, then as now
RGB_KERNEL_F16 = 'conv_f32_kernel<2, 2, 1, 1>'


def test_parsenet_f16_launch_census():
    """One ParseNet(128, 128) forward of 2 images per policy: under 'f16' EVERY convolution with whole 32-channel K steps is an x1 launch
    -- a layer the library refused would run on the base policy (exact f32) without a word -- the rest (the 3 -> 64 layer) runs the
    kernel it always ran, and the number of launches is the x3 policy's."""
    W = PN.synth_parsenet_state_dict(seed=0, in_size=128, out_size=128)
    x = nhwc(op_input('parsenet128', (2, 3, 128, 128)))
    census = {}
    for prec in ('f16', 'x3'):
        eng = PN.ParseNetEngine(W, in_size=128, out_size=128, precision=prec).to('cuda')
        eng.o.census = census[prec] = {}
        assert torch.isfinite(eng.logits_nhwc(x)).all()
    cins = []                                     # Cin of every convolution of engine.blocks
    for name, kind, cin, cout in eng.blocks:
        cins += [cin] if kind == 'conv' else [cin] * (2 if f'{name}.shortcut.weight' in eng.w else 1) + [cout]
    c16, c3 = census['f16'], census['x3']
    print('[f16-census] parsenet f16:', sorted(c16.items()), '\n[f16-census] parsenet x3 :', sorted(c3.items()))
    n_x1 = sum(1 for c in cins if c % 32 == 0)
    assert 0 < n_x1 == len(cins) - 1 and cins.count(3) == 1
    assert sum(n for k, n in c16.items() if k in X1_KERNELS) == n_x1
    assert sum(c16.values()) == sum(c3.values()) == len(cins)
    assert {k: n for k, n in c16.items() if k not in X1_KERNELS} == {RGB_KERNEL_F16: 1}
    assert not any(k in X1_KERNELS for k in c3)


def test_parsenet_f16_batch_of_16_equals_one_by_one():
    W = PN.synth_parsenet_state_dict(seed=0)
    eng = PN.ParseNetEngine(W, precision='f16').to('cuda')
    xb = torch.cat([op_input('parsenet512', (1, 3, 512, 512)), op_input('parsenet512_f16b', (15, 3, 512, 512))], 0).cuda()
    fp = PN.EngineFaceParse(eng)
    out = fp(xb)[0]
    assert out.shape == (16, 19, 512, 512)
    cls = eng.classes(ops.nchw_to_nhwc(xb))
    for i in range(16):
        assert torch.equal(fp(xb[i:i + 1])[0][0], out[i]), i
        assert torch.equal(eng.classes(ops.nchw_to_nhwc(xb[i:i + 1]))[0], cls[i]), i


def test_composite_1080p_3_faces_f16_vs_x3():
    from comfyui_keep_amd.engine import paste, synth
    frame, faces, mats, _ = synth.synth_paste_case()
    x = ((torch.from_numpy(faces[..., ::-1].copy()).float() / 255.0) - 0.5) / 0.5          # BGR uint8 crops -> the helper's normalised RGB, NHWC
    W = PN.synth_parsenet_state_dict(seed=0)
    cls = {p: PN.ParseNetEngine(W, precision=p).to('cuda').classes(x.cuda().contiguous()) for p in ('x3', 'f16')}
    gp = paste.GpuPaster('cuda')
    out = {p: gp.paste(frame, faces, list(mats), cls[p].cpu().numpy()).cpu().numpy().astype(np.int16) for p in ('x3', 'f16')}
    d = np.abs(out['f16'] - out['x3'])
    mx, share = int(d.max()), float((d != 0).any(-1).mean())
    print(f'[f16-composite] class maps differ in {int((cls["x3"] != cls["f16"]).sum())} of {cls["x3"].numel()} pixels; pasted 1080p frame: '
          f'max uint8 difference {mx}, share of differing pixels {share:.3e}')
    assert (out['x3'] != frame.astype(np.int16)).any()
    assert PASTE_MAX_MEASURED is not None, f'composite figures not recorded yet; measured max {mx}, share {share:.3e}'
    assert mx <= PASTE_MAX_MEASURED + 1


def test_default_path_is_x3_and_bit_equal(monkeypatch):
    """With KEEP_AMD_PARSE_PRECISION unset the loader builds an 'x3' engine whose class maps are those of a directly built one."""
    import sys
    import types
    if 'comfy' not in sys.modules:
        comfy, mm = types.ModuleType('comfy'), types.ModuleType('comfy.model_management')
        mm.get_torch_device = lambda: torch.device('cuda')
        mm.unet_offload_device = lambda: torch.device('cpu')
        mm.soft_empty_cache = lambda: None
        cu = types.ModuleType('comfy.utils')
        comfy.model_management, comfy.utils = mm, cu
        monkeypatch.setitem(sys.modules, 'comfy', comfy)
        monkeypatch.setitem(sys.modules, 'comfy.model_management', mm)
        monkeypatch.setitem(sys.modules, 'comfy.utils', cu)
        fpm = types.ModuleType('folder_paths')
        fpm.models_dir = '/nonexistent/models'
        monkeypatch.setitem(sys.modules, 'folder_paths', fpm)
    from comfyui_keep_amd.modules.keep_model_loader import engine_facelib
    monkeypatch.delenv('KEEP_AMD_PARSE_PRECISION', raising=False)
    W = PN.synth_parsenet_state_dict(seed=0)

    class Fake:
        def state_dict(self):
            return W

    class Hp:
        face_detector = None
    h = Hp()
    h.face_parse = Fake()
    engine_facelib(h)
    eng = h.face_parse.engine
    assert eng.precision == 'x3'
    eng.to('cuda')
    assert eng.o.mma == L.MMA_X3
    direct = PN.ParseNetEngine(W, precision='x3').to('cuda')
    x = nhwc(op_input('parsenet512', (1, 3, 512, 512)))
    assert torch.equal(eng.classes(x), direct.classes(x))
    assert torch.equal(eng.logits_nhwc(x), direct.logits_nhwc(x))
    safe = G['parsenet512_margin'].astype(np.float32) > 1e-2
    assert np.array_equal(eng.classes(x).cpu().numpy()[safe], G['parsenet512_classes'][safe])
