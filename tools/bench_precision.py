"""The KEEP network's precision policies side by side: frames/s of 'x3', 'f16' and 'bf16' (and, as extra rows, 'x3+up' / 'f16+up': the same
base with KEEP_AMD_UPSAMPLE_PRECISION=f16, the single-fp16 Upsample convolutions) for 1 and 16 clips per call at T = 20 -- rounds alternated
between the policies --, the
code-index agreement of 'f16' and 'bf16' with 'x3' over all frames, the share of the convolution FLOPs 'f16' runs on single-fp16
operands (counted from the plans of one forward), and a per-layer A/B of the X1 GroupNorm-swish kernel against the x3 kernel.

One process, synthetic weights and clips (engine/synth.py), wall time around synchronised calls for the network (a B = 1 call is a graph
replay), HIP events and interleaved rounds for the per-layer A/B.  Prints one JSON line per measurement.  Run every invocation under a
time limit of its own, e.g. ``timeout -k 10 900 python tools/bench_precision.py``."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_keep_amd.engine import hiplib as L  # noqa: E402
from comfyui_keep_amd.engine import ops, synth  # noqa: E402
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH  # noqa: E402
from comfyui_keep_amd.engine.net import KeepNet  # noqa: E402

GFLOP_PER_FRAME = 1038.5      # algorithmic FLOPs of one 512 x 512 frame
X1_FORMS = ('conv3x3_halo_x3s_kernel<0, false, true>', 'conv3x3_halo_x3s_kernel<0, true, true>', 'conv3x3_halo_x3s_kernel<1, true, true>',
            'conv3x3_halo_x3s_kernel<2, true, true>', ops.X1_UP2_KERNEL)


def network(a):
    W = synth.synth_state_dict(seed=0)
    T = a.frames
    clips = {b: synth.synth_clip(T=T, B=b, seed=1234).cuda() for b in a.clips}
    idx, nets = {}, {}
    for prec in a.precisions:      # 'x3+up': base 'x3' with the Upsample knob on
        net = nets[prec] = KeepNet(**DEFAULT_ARCH)
        net.load_state_dict(W, strict=True)
        net.to('cuda').eval().set_precision(prec.split('+')[0]).set_upsample_precision('f16' if prec.endswith('+up') else 'x3')
    for b in a.clips:              # every round visits every policy once: drift of the box hits all of them alike
        x = clips[b]
        for net in nets.values():
            for _ in range(a.warmup):
                net(x)
        torch.cuda.synchronize()
        s = {prec: [] for prec in nets}
        for _ in range(a.reps):
            for prec, net in nets.items():
                t0 = time.perf_counter()
                net(x)
                torch.cuda.synchronize()
                s[prec].append(time.perf_counter() - t0)
        for prec, net in nets.items():
            med = statistics.median(s[prec])
            print(json.dumps({'bench': 'keep_forward', 'precision': prec, 'clips': b, 'T': T, 'median_s': round(med, 4), 'min_s': round(min(s[prec]), 4),
                              'max_s': round(max(s[prec]), 4), 'frames_per_s': round(b * T / med, 1), 'reps': a.reps, 'fallbacks': net.x3_fallbacks}), flush=True)
    for prec, net in nets.items():
        _, aux = net(clips[max(a.clips)], return_aux=True)
        idx[prec] = aux['indices'].cpu()
        if prec.split('+')[0] == 'f16':      # what runs on single fp16: one profiled forward of one clip, FLOPs by the plan's kernel name
            net.o.profile = []
            net(clips[min(a.clips)][:1], return_aux=True)
            torch.cuda.synchronize()
            by = {}
            for rec in net.o.profile:
                by[rec[0]] = by.get(rec[0], 0.0) + rec[1]
            net.o.profile = None
            x1 = sum(v for k, v in by.items() if k in X1_FORMS)
            print(json.dumps({'bench': 'f16_flop_share', 'precision': prec, 'x1_gflop_per_frame': round(x1 / T / 1e9, 1),
                              'x3_streaming_gflop_per_frame_left': round(by.get(ops.X3_STREAM_KERNEL, 0.0) / T / 1e9, 1),
                              'conv_gflop_per_frame': round(sum(by.values()) / T / 1e9, 1), 'share_of_conv_flops': round(x1 / sum(by.values()), 4),
                              'share_of_1038.5_gflop': round(x1 / T / 1e9 / GFLOP_PER_FRAME, 4),
                              'by_kernel_gflop_per_frame': {k: round(v / T / 1e9, 2) for k, v in sorted(by.items(), key=lambda kv: -kv[1])}}), flush=True)
    for prec in a.precisions:
        if prec != 'x3' and 'x3' in idx:
            agree = (idx[prec] == idx['x3']).float()
            print(json.dumps({'bench': 'code_index_agreement_with_x3', 'precision': prec, 'clips': max(a.clips), 'T': T, 'all_frames': round(float(agree.mean()), 5),
                              'frame0': round(float(agree[:, 0].mean()), 5), 'last_frame': round(float(agree[:, -1].mean()), 5)}), flush=True)


def per_layer(a):
    """conv3x3 behind GroupNorm + swish with fused statistics (a VQGAN ResBlock convolution), 16 images: the X1 form against the x3 form,
    interleaved rounds in one process."""
    g = torch.Generator().manual_seed(0)
    for C, hw in ((64, 512), (128, 256)):
        n = 16
        x = torch.randn((n, hw, hw, C), generator=g).cuda()
        w = (torch.randn((C, 3, 3, C), generator=g) / (3.0 * C ** 0.5)).cuda()
        b = torch.randn((C,), generator=g).cuda() * 0.1
        pro = ((0.5 + torch.rand((n, C), generator=g)).cuda(), (torch.randn((n, C), generator=g) * 0.3).cuda())
        sw = ops.x3_scale_for(float(w.abs().max()))
        forms = {'x3': dict(mma=L.MMA_X3, wx3=ops.split_x3(w.reshape(-1, C), sw).view(-1)),
                 'x1': dict(mma=L.MMA_X1, wx3=(w.reshape(-1) * sw).to(torch.float16).view(torch.int16))}
        out = torch.empty((n, hw, hw, C), device='cuda')
        ms = {k: [] for k in forms}
        names = {}
        for r in range(a.warmup + a.reps):
            for k, kw in forms.items():
                ops.DEFAULT.profile = []
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.conv(x, w, b, pro=pro, pro_act=L.PRO_SWISH, x3_acc_scale=1.0 / sw, stats=True, out=out, **kw)
                e1.record()
                e1.synchronize()
                names[k] = ops.DEFAULT.profile[-1][0]
                ops.DEFAULT.profile = None
                if r >= a.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        flop = 2.0 * n * hw * hw * C * C * 9
        rec = {'bench': 'conv3x3_gn_swish_ab', 'channels': C, 'map': hw, 'images': n}
        for k in forms:
            med = statistics.median(ms[k])
            rec[k] = {'kernel': names[k], 'median_ms': round(med, 4), 'min_ms': round(min(ms[k]), 4), 'tflops': round(flop / med / 1e9, 1)}
        rec['x1_over_x3'] = round(statistics.median(ms['x3']) / statistics.median(ms['x1']), 3)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precisions', nargs='+', default=['x3', 'f16', 'bf16'], help="base policies; 'x3+up' / 'f16+up' add the Upsample knob")
    ap.add_argument('--clips', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-network', action='store_true')
    ap.add_argument('--skip-layers', action='store_true')
    a = ap.parse_args()
    print(json.dumps({'bench': 'precision', 'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d')}), flush=True)
    if not a.skip_layers:
        per_layer(a)
    if not a.skip_network:
        network(a)


if __name__ == '__main__':
    main()
