"""GMFlow's opt-in single-fp16 precision (KEEP_AMD_FLOW_PRECISION=f16) beside the policies it rides on, in one process on one box:

(a) the window-attention launch of GMFlow at 16 clips, T = 20 (608 images of 64 x 64 tokens, 1024-token windows, cross-attention layout):
    KEEP_MMA_X1 | KEEP_ATTN_X1 against the x3 packed form, HIP events, interleaved rounds, microseconds per launch;
(b) the time of ``_gmflow_clip`` and of the whole forward at 16 clips and at 1 clip under 'x3', 'f16', 'x3 + flow f16' and 'f16 + flow f16'
    -- the settings alternate, two passes, the SECOND pass is reported -- and, from one profiled ``_gmflow_clip`` per setting, every
    convolution launch shape of GMFlow that flow 'f16' moves to a single-fp16 kernel with its time under either policy;
(c) the flow error on tests/golden/gmflow256.npz and the pixel error on the T = 3 golden with the reference's indices injected (the
    figures tests/test_gpu_flow_f16.py holds as dated constants).

Synthetic weights and clips (engine/synth.py).  Prints one JSON line per measurement.  Run every invocation under a time limit of its own,
e.g. ``timeout -k 10 900 python tools/bench_flow_precision.py``."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_keep_amd.engine import hiplib as L  # noqa: E402
from comfyui_keep_amd.engine import ops, synth  # noqa: E402
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH  # noqa: E402
from comfyui_keep_amd.engine.net import KeepNet  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SETTINGS = (('x3', 'x3', 'x3'), ('f16', 'f16', 'x3'), ('x3 + flow f16', 'x3', 'f16'), ('f16 + flow f16', 'f16', 'f16'))


def window_attention(a):
    C, h8, P = 128, 64, a.clips * (a.frames - 1)
    n_img, Lt = 2 * P, h8 * h8
    g = torch.Generator().manual_seed(0)
    q = torch.randn((n_img * Lt, C), generator=g).cuda()
    kv = torch.randn((n_img * Lt, 2 * C), generator=g).cuda()
    o = torch.empty((n_img * Lt, C), device='cuda')
    forms = {'x3': (L.MMA_X3, 0), 'x1': (L.MMA_X1, L.ATTN_X1)}
    for shift in (0, h8 // 4):
        kw = dict(q=q, k=kv, v=ops.offset(kv, C), o=o, B=n_img * 4, H=1, Lq=Lt // 4, Lk=Lt // 4, D=C, Dv=C, scale=1.0 / math.sqrt(C), mode=2,
                  img_h=h8, img_w=h8, ksplit=2, shift=shift, kv_rot=P, n_img=n_img, in_dtype=L.F32,
                  q_bs=Lt * C, q_ts=C, q_hs=0, k_bs=Lt * 2 * C, k_ts=2 * C, k_hs=0, v_bs=Lt * 2 * C, v_ts=2 * C, v_hs=0, o_bs=Lt * C, o_ts=C, o_hs=0)
        us = {k: [] for k in forms}
        ws = {}
        for r in range(a.warmup + a.reps):
            for k, (mma, flags) in forms.items():
                args = dict(kw, mma=mma, flags=flags)
                ws[k] = L.attention_workspace_bytes(L.attn_args(**args))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.attention(**args)
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    us[k].append(1e3 * e0.elapsed_time(e1))
        flop = 4.0 * n_img * 4 * (Lt // 4) ** 2 * C
        rec = {'bench': 'window_attention_ab', 'clips': a.clips, 'T': a.frames, 'images': n_img, 'window_tokens': Lt // 4, 'shift': shift}
        for k in forms:
            med = statistics.median(us[k])
            rec[k] = {'median_us': round(med, 1), 'min_us': round(min(us[k]), 1), 'tflops': round(flop / med / 1e6, 1), 'workspace_MiB': round(ws[k] / 2 ** 20, 1)}
        rec['x1_over_x3'] = round(statistics.median(us['x3']) / statistics.median(us['x1']), 3)
        print(json.dumps(rec), flush=True)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    return statistics.median(s), min(s)


def flow_only(net, x):
    with torch.cuda.device(net.device):
        net._activate_precision()
        net.o.begin_forward(net.device)
        if net.of is not net.o:
            net.of.begin_forward(net.device)
        return net._gmflow_clip(x)


def network(a, W):
    nets = {}
    for name, base, flow in SETTINGS:
        net = KeepNet(**DEFAULT_ARCH)
        net.load_state_dict(W, strict=True)
        nets[name] = net.to('cuda').eval().set_precision(base).set_flow_precision(flow)
    T = a.frames
    for b in (a.clips, 1):
        x = synth.synth_clip(T=T, B=b, seed=1234).cuda()
        for p in range(2):      # the settings alternate; the second pass is the one reported
            for name, net in nets.items():
                gm, gm_min = timed(lambda: flow_only(net, x), a.warmup if p == 0 else 1, a.reps)
                fw, fw_min = timed(lambda: net(x), a.warmup if p == 0 else 1, a.reps)
                if p == 1:
                    print(json.dumps({'bench': 'keep_forward', 'setting': name, 'clips': b, 'T': T, 'gmflow_clip_ms': round(1e3 * gm, 2), 'gmflow_clip_min_ms': round(1e3 * gm_min, 2),
                                      'forward_s': round(fw, 4), 'forward_min_s': round(fw_min, 4), 'frames_per_s': round(b * T / fw, 1), 'reps': a.reps,
                                      'fallbacks': net.x3_fallbacks}), flush=True)
        if b == a.clips:      # per launch shape: one profiled _gmflow_clip under x3 and under x3 + flow f16, summed HIP-event times per shape
            by = {}
            for name in ('x3', 'x3 + flow f16'):
                net = nets[name]
                for rep in range(3):
                    net.o.profile = []
                    flow_only(net, x)
                    torch.cuda.synchronize()
                    prof, net.o.profile = net.o.profile, None
                    if net.of is not net.o:
                        net.of.profile = None
                    if rep == 0:
                        continue
                    for rec in prof:
                        d = by.setdefault(rec[6], {}).setdefault(name, {'kernel': rec[0], 'ms': [], 'launches': 0})
                        d['ms'].append(rec[3].elapsed_time(rec[4]))
                        d['launches'] += 1
            for shape, d in by.items():
                if 'x3' in d and 'x3 + flow f16' in d and d['x3']['kernel'] != d['x3 + flow f16']['kernel']:
                    t3, t1 = (sum(d[k]['ms']) / 2 for k in ('x3', 'x3 + flow f16'))
                    print(json.dumps({'bench': 'gmflow_conv_shape_ab', 'clips': b, 'shape_N_H_W_Cin_Cout_k_stride_up_pro': list(shape), 'launches': d['x3']['launches'] // 2,
                                      'x3': {'kernel': d['x3']['kernel'], 'ms': round(t3, 3)}, 'x1': {'kernel': d['x3 + flow f16']['kernel'], 'ms': round(t1, 3)},
                                      'x1_over_x3': round(t3 / t1, 3)}), flush=True)
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-attention', action='store_true')
    ap.add_argument('--skip-network', action='store_true')
    a = ap.parse_args()
    print(json.dumps({'bench': 'flow_precision', 'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d')}), flush=True)
    if not a.skip_attention:
        window_attention(a)
    if not a.skip_network:
        W = synth.synth_state_dict(seed=0)
        errors(network(a, W), W)


if __name__ == '__main__':
    main()
