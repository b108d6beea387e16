"""SHA-256 of what keep_conv2d writes, one process per library (needs the GPU): every launched CONV_CASES entry of
tests/test_gpu_footprint.py through footprint.plain, plus the x1 forms and three launch-time switches that table does not reach.  Per case
the plan's kernel and the hash of every returned window (out, statistics, amax arena, split-K workspace).

    python tools/dev/conv_case_hashes.py LIB.so OUT.json

Two libraries compute alike when the two JSON files are equal; under ``rocprofv3 --kernel-trace -- python ...`` the same run gives the
ordered launches (profiles/conv_plan_refactor.txt)."""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if __name__ == '__main__':
    os.environ['KEEP_HIP_LIB'] = os.path.abspath(sys.argv[1])
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
from __graft_entry__ import load_package
load_package()
import torch
import footprint as FP
import test_gpu_footprint as T
from conftest import op_input
from comfyui_keep_amd.engine import hiplib as L, ops

X3, X1 = L.MMA_X3, L.MMA_X1
# name -> geometry (3x3 stride-1 pad-1 unless k / stride say otherwise), one shape each from tests/test_gpu_conv_x1_*.py and the smallest
# shapes that reach the statistics replica, the small tile for few rows and the M > 262144 shallow form
EXTRA = {
    'x1_stream_raw': dict(mma=X1, N=1, H=8, W=32, Cin=32, Cout=32),
    'x1_stream_affine': dict(mma=X1, N=1, H=8, W=32, Cin=32, Cout=32, pro=True),
    'x1_stream_relu': dict(mma=X1, N=1, H=8, W=32, Cin=32, Cout=32, pro=True, pro_act=L.PRO_RELU),
    'x1_stream_swish': dict(mma=X1, N=1, H=8, W=32, Cin=32, Cout=32, pro=True, pro_act=L.PRO_SWISH),
    # the streaming kernel with an epilogue activation (conv3x3_halo_x3s_act_kernel): the detectors' SiLU / LeakyReLU(0.1), ReLU, one behind a prologue;
    # CONV_NO_SMALL_PARTIALS keeps launches of so few items on the 256-pixel kernel
    'x3s_silu': dict(mma=X3, N=2, H=8, W=32, Cin=32, Cout=64, act=L.ACT_SILU, split_k=1, stats=True, flags=L.CONV_NO_SMALL_PARTIALS),
    'x3s_relu': dict(mma=X3, N=1, H=8, W=32, Cin=32, Cout=64, act=L.ACT_RELU, split_k=1, stats=True, flags=L.CONV_NO_SMALL_PARTIALS),
    'x3s_lrelu01': dict(mma=X3, N=1, H=8, W=32, Cin=48, Cout=64, act=L.ACT_LRELU01, split_k=1, flags=L.CONV_NO_SMALL_PARTIALS),
    'x3s_gelu': dict(mma=X3, N=1, H=8, W=32, Cin=32, Cout=64, act=L.ACT_GELU, split_k=1, flags=L.CONV_NO_SMALL_PARTIALS),
    'x3s_swish_lrelu01': dict(mma=X3, N=1, H=8, W=32, Cin=32, Cout=64, pro=True, pro_act=L.PRO_SWISH, act=L.ACT_LRELU01, split_k=1, stats=True,
                              flags=L.CONV_NO_SMALL_PARTIALS),
    'x1_stream_silu': dict(mma=X1, N=2, H=8, W=32, Cin=32, Cout=64, act=L.ACT_SILU),
    'x1_stream_relu': dict(mma=X1, N=1, H=8, W=32, Cin=32, Cout=64, act=L.ACT_RELU),
    'x1_halo16': dict(mma=X1, N=16, H=16, W=16, Cin=32, Cout=32, flags=L.CONV_X1_HALO16),
    'x1_halo16_act': dict(mma=X1, N=16, H=16, W=16, Cin=32, Cout=32, flags=L.CONV_X1_HALO16, act=L.ACT_SILU),
    'x1_im2col_s2': dict(mma=X1, N=2, H=16, W=16, Cin=32, Cout=64, stride=2),
    'x1_gemm_t1': dict(mma=X1, N=2, H=64, W=1, Cin=32, Cout=64, k=1, flags=L.CONV_X1_GEMM),
    'x1_gemm_t2': dict(mma=X1, N=5, H=1025, W=1, Cin=256, Cout=256, k=1, flags=L.CONV_X1_GEMM),
    'gather_stats_replica': dict(mma=X3, N=1, H=64, W=64, Cin=16, Cout=128, stride=2, split_k=1, stats=True),
    'gather_small_tile': dict(mma=X3, N=1, H=64, W=64, Cin=16, Cout=128, stride=2, split_k=1),
    'gather_shallow': dict(mma=X3, N=1, H=1040, W=1040, Cin=16, Cout=32, stride=2),
    # the x2-phase Upsample (phase weights, output 2H x 2W): three cout blocks with inner tile edges, 640 items on <= 512 blocks (item seams,
    # image boundaries), and the stage-barrier form of the first under KEEP_CONV_NO_STREAM on the same data (`data`) -- the same hashes as its twin
    'up2_three_blocks': dict(mma=X3, N=1, H=16, W=64, Cin=32, Cout=192, up2=True, split_k=1, stats=True),
    'up2_item_seams': dict(mma=X3, N=5, H=64, W=64, Cin=32, Cout=256, up2=True, split_k=1, stats=True),
    'up2_three_blocks_no_stream': dict(mma=X3, N=1, H=16, W=64, Cin=32, Cout=192, up2=True, split_k=1, stats=True, flags=L.CONV_NO_STREAM,
                                       data='up2_three_blocks'),
}


def extra_case(name):
    c = dict(k=3, stride=1, pro=False, pro_act=L.PRO_NONE, act=L.ACT_NONE, flags=0, stats=False, split_k=0, up2=False)      # (split_k = 1: the caller asks for a single pass, as it does when it wants statistics)
    c.update(EXTRA[name])
    name = c.get('data', name)      # (the inputs are generated from the case's name)
    k, s, N, H, W, Cin, Cout = c['k'], c['stride'], c['N'], c['H'], c['W'], c['Cin'], c['Cout']
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    x = op_input('cch:' + name + 'x', (N * H * W, Cin), 2.0) + 0.3
    w = op_input('cch:' + name + 'w', (Cout, k, k, Cin), 0.05)
    sc = ops.x3_scale_for(float(w.abs().max()))
    if c['up2']:
        Ho, Wo = 2 * H, 2 * W
        w4 = ops.up2_phase_weights(w)
        sc = ops.x3_scale_for(float(w4.abs().max()))
        twin = ops.split_x3(w4.reshape(-1, Cin), sc).reshape(4 * Cout, -1)
    else:
        twin = (w * sc).to(torch.float16).reshape(Cout, -1) if c['mma'] == X1 else ops.split_x3(w.reshape(-1, Cin), sc).reshape(Cout, -1)
    amax = x.reshape(N, -1).abs().amax(1) * (1.2 if c['pro'] else 1.0) + (0.2 if c['pro'] else 0.0)      # (an upper bound of what the prologue gives)
    R = [FP.single('x', x), FP.single('w', w.reshape(Cout, -1)), FP.single('bias', op_input('cch:' + name + 'b', (1, Cout))),
         FP.single('wx3', twin.contiguous()), FP.single('in_amax', amax.reshape(1, N)), FP.output('out', (N * Ho * Wo, Cout))]
    if c['pro']:
        R += [FP.single('pro_scale', op_input('cch:' + name + 'ps', (N, Cin)) * 0.2 + 1), FP.single('pro_shift', op_input('cch:' + name + 'ph', (N, Cin)) * 0.2)]

    def args(t):
        p = {n: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for n, v in t.items()}
        return L.conv_args(inp=p['x'], weight=p['w'], bias=p['bias'], out=p['out'], pro_scale=p.get('pro_scale'), pro_shift=p.get('pro_shift'),
                           workspace=p.get('ws'), stats_out=p.get('stats'), stats_P=t.get('stats_P', 0), N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=k, KW=k,
                           stride=s, pad_t=pad, pad_l=pad, Ho=Ho, Wo=Wo, in_ld=Cin, out_ld=Cout, pro_act=c['pro_act'], epi_act=c['act'], mma=c['mma'],
                           weight_x3=p['wx3'], x3_acc_scale=1.0 / sc, x3_in_amax=p['in_amax'], flags=c['flags'], split_k=c['split_k'],
                           upsample=L.UPSAMPLE_X2_PHASES if c['up2'] else 0)
    plan = L.conv2d_plan(args({n: 0x10000 for r in R for n in r.windows}))
    extra = {}
    if plan.split_k > 1:
        R.append(FP.output('ws', (1, plan.workspace_bytes // 4)))
    if c['stats']:
        assert plan.stats_P > 0, name
        R.append(FP.output('stats', (1, N * plan.stats_P * Cout * 2)))
        extra['stats_P'] = plan.stats_P
    return plan, R, lambda t: args({**t, **extra})


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    rows = {}
    for name, (_, _, kw) in T.CONV_CASES.items():
        if not kw.get('launch', True): continue
        g, plan, regions, extra = T._conv_regions(name)
        for r in regions: r.compare = True      # (the split-K workspace too)
        def launch(t, g=g, extra=extra):
            a = T._conv_args(g, {**t, **extra})
            a.split_k = L.conv2d_plan(a).split_k
            L.conv2d_launch(a)
        outs, _ = FP.plain(launch, regions, 'cuda')
        rows[name] = {'kernel': plan.kernel.decode(), **{n: sha(v) for n, v in sorted(outs.items())}}
    for name in EXTRA:
        plan, regions, args = extra_case(name)
        def launch(t, args=args):
            a = args(t)
            a.split_k = L.conv2d_plan(a).split_k
            L.conv2d_launch(a)
        outs, _ = FP.plain(launch, regions, 'cuda')
        rows['extra:' + name] = {'kernel': plan.kernel.decode(), 'split_k': plan.split_k, **{n: sha(v) for n, v in sorted(outs.items())}}
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    json.dump(rows, open(sys.argv[2], 'w'), indent=1, sort_keys=True)
    print(len(rows), 'cases', hashlib.sha256(json.dumps(rows, sort_keys=True).encode()).hexdigest())


if __name__ == '__main__':
    main()
