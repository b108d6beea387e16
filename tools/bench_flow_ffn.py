"""GMFlow's fused feed-forward block on single fp16 (KEEP_AMD_FLOW_FFN_PRECISION=f16, keep_gm_ffn_x1) beside the x3 entry it replaces, in one
process on one box:

(a) the kernel: keep_gm_ffn_x1 against keep_gm_ffn_x3 at GMFlow's token counts (16 clips x T = 20: M = 2 490 368; one clip: M = 155 648;
    C = 128, hidden = 1024), HIP events, the two entries interleaved, two passes, median of ``--reps`` of the SECOND pass, both GELU forms;
(b) ``_gmflow_clip`` and the whole forward at 16 clips and at 1 clip under 'x3', 'f16', 'x3 + flow f16' and 'f16 + flow f16', each without
    and with the FFN knob -- the settings alternate, two passes, the second pass is reported;
(c) the flow error on tests/golden/gmflow256.npz and the pixel error on the T = 3 golden with the reference's indices injected, per setting
    (the figures tests/test_gpu_flow_ffn_f16.py holds as dated constants).

Synthetic weights and clips (engine/synth.py).  Prints one JSON line per measurement.  Run every invocation under a time limit of its own,
e.g. ``timeout -k 10 900 python tools/bench_flow_ffn.py``."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_flow_precision import GOLDEN, SETTINGS, flow_only, timed  # noqa: E402  (loads the package)
from comfyui_keep_amd.engine import hiplib as L  # noqa: E402
from comfyui_keep_amd.engine import ops, synth  # noqa: E402
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH  # noqa: E402
from comfyui_keep_amd.engine.net import KeepNet  # noqa: E402

C, HIDDEN = 128, 1024


def kernel_ab(a):
    g = torch.Generator().manual_seed(0)
    w0, w2 = 0.08 * torch.randn((HIDDEN, 2 * C), generator=g), 0.05 * torch.randn((C, HIDDEN), generator=g)
    w2p = ops.ffn_w2_perm(w2)
    s0, s2 = ops.x3_scale_for(float(w0.abs().max())), ops.x3_scale_for(float(w2p.abs().max()))
    twins = {'x3': ('keep_gm_ffn_x3', ops.split_x3(w0, s0).cuda(), ops.split_x3(w2p, s2).cuda()),
             'x1': ('keep_gm_ffn_x1', (w0 * s0).to(torch.float16).view(torch.int16).cuda(), (w2p * s2).to(torch.float16).view(torch.int16).cuda())}
    gamma, beta = (1.0 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.2 * torch.randn(C, generator=g)).cuda()
    for M in (a.clips * (a.frames - 1) * 2 * 64 * 64, (a.frames - 1) * 2 * 64 * 64):
        src, msg = 1.5 * torch.randn((M, C), device='cuda'), torch.randn((M, C), device='cuda')
        out = torch.empty((M, C), device='cuda')
        for exact in (0, 1):
            us = {k: [] for k in twins}
            for p in range(2):      # the second pass is the one reported
                for r in range(a.reps):
                    for k, (sym, t0, t2) in twins.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        L.call(sym, src, msg, t0, 1.0 / s0, t2, 1.0 / s2, gamma, beta, 1e-5, out, M, C, HIDDEN, exact)
                        e1.record()
                        e1.synchronize()
                        if p == 1:
                            us[k].append(1e3 * e0.elapsed_time(e1))
            flop = 2.0 * M * (2 * C * HIDDEN + HIDDEN * C)
            rec = {'bench': 'gm_ffn_kernel_ab', 'M': M, 'C': C, 'hidden': HIDDEN, 'exact_act': exact, 'reps': a.reps}
            for k in twins:
                med = statistics.median(us[k])
                rec[k] = {'median_us': round(med, 1), 'min_us': round(min(us[k]), 1), 'tflops': round(flop / med / 1e6, 1)}
            rec['x1_over_x3'] = round(statistics.median(us['x3']) / statistics.median(us['x1']), 3)
            print(json.dumps(rec), flush=True)
        del src, msg, out


def network(a, W):
    nets = {}
    for name, base, flow in SETTINGS:
        for ffn in ('x3', 'f16'):
            net = KeepNet(**DEFAULT_ARCH)
            net.load_state_dict(W, strict=True)
            nets[name + (' + ffn f16' if ffn == 'f16' else '')] = net.to('cuda').eval().set_precision(base).set_flow_precision(flow).set_flow_ffn_precision(ffn)
    T = a.frames
    for b in (a.clips, 1):
        x = synth.synth_clip(T=T, B=b, seed=1234).cuda()
        for p in range(2):      # the settings alternate; the second pass is the one reported
            for name, net in nets.items():
                gm, gm_min = timed(lambda: flow_only(net, x), a.warmup if p == 0 else 1, a.net_reps)
                fw, fw_min = timed(lambda: net(x), a.warmup if p == 0 else 1, a.net_reps)
                if p == 1:
                    print(json.dumps({'bench': 'keep_forward', 'setting': name, 'clips': b, 'T': T, 'gmflow_clip_ms': round(1e3 * gm, 2), 'gmflow_clip_min_ms': round(1e3 * gm_min, 2),
                                      'forward_s': round(fw, 4), 'forward_min_s': round(fw_min, 4), 'frames_per_s': round(b * T / fw, 1), 'reps': a.net_reps,
                                      'fallbacks': net.x3_fallbacks}), flush=True)
    return nets


def errors(nets, W):
    g = np.load(os.path.join(GOLDEN, 'gmflow256.npz'))
    dt = int(g['dt'])
    a = synth.synth_clip(T=dt + 1, B=1, size=256, seed=int(g['clip_seed']))[0]
    bf = KeepNet(**DEFAULT_ARCH)
    bf.load_state_dict(W, strict=True)
    nets = dict(nets, bf16=bf.to('cuda').eval().set_precision('bf16'))
    rec = {'bench': 'gmflow256_flow_error_px', 'scale_px': round(float(np.abs(g['flow']).max()), 2)}
    for name, net in nets.items():
        with torch.cuda.device(net.device):
            net._activate_precision()
            flow = net._gmflow(a[dt:dt + 1].cuda(), a[0:1].cuda()).permute(0, 3, 1, 2).cpu().numpy()
        e = np.sqrt(((flow - g['flow']) ** 2).sum(1))
        rec[name] = {'max': float(f'{np.abs(flow - g["flow"]).max():.4e}'), 'median': float(f'{np.median(e):.4e}')}
    print(json.dumps(rec), flush=True)
    g = np.load(os.path.join(GOLDEN, 'keep_forward_T3.npz'))
    x = synth.synth_clip(T=3, B=1, seed=1234).cuda()
    forced = torch.from_numpy(g['indices'].astype(np.int32)).view(1, 3, -1)
    rec = {'bench': 'keep_forward_T3_pixel_error', 'output_scale': round(float(np.abs(g['out_grid']).max()), 3)}
    for name, net in nets.items():
        out = net(x, force_indices=forced)[0].cpu()
        H, Wd = out.shape[2:]
        rec[name] = float(f'{np.abs(out[:, :, 7::H // 32, 5::Wd // 32][:, :, :32, :32].numpy() - g["out_grid"]).max():.4e}')
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=16)
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5, help='kernel A/B launches per entry and pass')
    ap.add_argument('--net-reps', type=int, default=5, help='timed runs per setting and pass')
    ap.add_argument('--skip-kernel', action='store_true')
    ap.add_argument('--skip-network', action='store_true')
    a = ap.parse_args()
    print(json.dumps({'bench': 'flow_ffn', 'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d')}), flush=True)
    if not a.skip_kernel:
        kernel_ab(a)
    if not a.skip_network:
        W = synth.synth_state_dict(seed=0)
        errors(network(a, W), W)


if __name__ == '__main__':
    main()
