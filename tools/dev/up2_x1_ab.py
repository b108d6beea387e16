#!/usr/bin/env python
"""The generator's Upsample convolutions, three forms alternated in ONE process (profiles/f16_upsample_precision.txt (a)):
  x3 phases   KEEP_MMA_X3, upsample = KEEP_UPSAMPLE_X2_PHASES (conv3x3_up2_x3s_kernel)
  x1 phases   KEEP_MMA_X1 | KEEP_CONV_X1_UP2 on the hi-only phase twin (conv3x3_up2_x1s_kernel)
  x1 up1      KEEP_MMA_X1, upsample = 1 on the hi-only twin (conv3x3_halo_x3s_kernel<0, false, true>: nine taps, no new kernel)
as the network launches them: bias, statistics partials, max|out|, the producer's max|x| as range probe.  HIP events around each launch,
ITERS launches per form and round, ROUNDS rounds; prints one JSON line per shape with the medians over the rounds and x3's own spread.
   python tools/dev/up2_x1_ab.py [layer ...]      (layers of tools/bench_conv.py whose name starts with `up`)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_keep_amd.engine import hiplib as L  # noqa: E402
from comfyui_keep_amd.engine import ops  # noqa: E402
from bench_conv import LAYERS  # noqa: E402

ITERS, ROUNDS = int(os.environ.get('ITERS', '10')), int(os.environ.get('ROUNDS', '7'))


def main():
    names = sys.argv[1:] or ['up128_512_n48', 'up128_256_n48', 'up256_128_n48', 'up256_64_n48', 'up128_512_n1']
    for name in names:
        N, H, W, Cin, Cout, k, up = LAYERS[name]
        assert up and k == 3, name
        g = torch.Generator().manual_seed(1)
        x = torch.randn((N, H, W, Cin), generator=g).cuda()
        w = (torch.randn((Cout, 3, 3, Cin), generator=g) * 0.05).cuda()
        b = torch.randn((Cout,), generator=g).cuda()
        amax = x.reshape(N, -1).abs().amax(1).contiguous()
        out = torch.empty((N, 2 * H, 2 * W, Cout), device='cuda')
        w4 = ops.up2_phase_weights(w)
        s4, s1 = ops.x3_scale_for(float(w4.abs().max())), ops.x3_scale_for(float(w.abs().max()))
        forms = {
            'x3_phases': (0, dict(mma=L.MMA_X3, upsample=L.UPSAMPLE_X2_PHASES, wx3=ops.split_x3(w4.reshape(-1, Cin), s4).view(-1), x3_acc_scale=1.0 / s4)),
            'x1_phases': (L.CONV_X1_UP2, dict(mma=L.MMA_X1, upsample=L.UPSAMPLE_X2_PHASES,
                                              wx3=(w4.reshape(-1) * s4).to(torch.float16).view(torch.int16), x3_acc_scale=1.0 / s4)),
            'x1_up1': (0, dict(mma=L.MMA_X1, upsample=True, wx3=(w.reshape(-1) * s1).to(torch.float16).view(torch.int16), x3_acc_scale=1.0 / s1)),
        }
        o = ops.Ops()
        us = {f: [] for f in forms}
        kern = {}
        for r in range(ROUNDS + 1):      # round 0 warms up
            for f, (flags, kw) in forms.items():
                o.flags = flags
                o.profile = []
                for _ in range(ITERS):
                    o.conv(x, w, b, stats=True, x_amax=amax, out=out, **kw)
                torch.cuda.synchronize()
                rec, o.profile = o.profile, None
                kern[f] = rec[0][0]
                if r:
                    us[f].append(1e3 * statistics.median(e[3].elapsed_time(e[4]) for e in rec))
        flop = 2.0 * N * 4 * H * W * Cout * 9 * Cin      # algorithmic: nine taps per output pixel
        row = {'bench': 'up2_x1_ab', 'layer': name, 'N': N, 'source': [H, W], 'Cin': Cin, 'Cout': Cout, 'iters': ITERS, 'rounds': ROUNDS}
        for f in forms:
            med = statistics.median(us[f])
            row[f] = {'kernel': kern[f], 'median_us': round(med, 1), 'min_us': round(min(us[f]), 1), 'max_us': round(max(us[f]), 1),
                      'alg_tflops': round(flop / med / 1e6, 1)}
        x3 = row['x3_phases']
        row['x3_round_spread'] = round((x3['max_us'] - x3['min_us']) / x3['median_us'], 4)
        row['x1_phases_over_x3'] = round(x3['median_us'] / row['x1_phases']['median_us'], 3)
        row['x1_up1_over_x3'] = round(x3['median_us'] / row['x1_up1']['median_us'], 3)
        print(json.dumps(row), flush=True)
        del x, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
