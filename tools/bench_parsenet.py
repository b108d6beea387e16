"""ParseNet(512, 512) on the engine: faces/s of ``engine.classes`` for 1, 16 and 32 faces under the 'x3' and 'f16' policies.

One process, synthetic weights, HIP-event time: per (policy, batch) WARMUP calls, then REPS timed calls, the median is reported.
Prints one JSON line per measurement and a closing summary line.  Run every invocation under a time limit of its own, e.g.
``timeout -k 10 300 python tools/bench_parsenet.py``."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_keep_amd.engine import parsenet as PN  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--faces', type=int, nargs='+', default=[1, 16, 32])
    ap.add_argument('--precisions', nargs='+', default=['x3', 'f16'])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=15)
    a = ap.parse_args()
    W = PN.synth_parsenet_state_dict(seed=0)
    g = torch.Generator().manual_seed(0)
    summary = {}
    for prec in a.precisions:
        eng = PN.ParseNetEngine(W, precision=prec).to('cuda')
        for n in a.faces:
            x = (torch.rand((n, 512, 512, 3), generator=g) * 2 - 1).cuda()
            for _ in range(a.warmup):
                eng.classes(x)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.classes(x)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            rec = {'precision': prec, 'faces': n, 'median_ms': round(med, 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3),
                   'faces_per_s': round(n / med * 1e3, 1), 'reps': a.reps}
            summary[f'{prec}_{n}'] = rec['faces_per_s']
            print(json.dumps(rec), flush=True)
        del eng
    print(json.dumps({'bench': 'parsenet_classes', 'device': torch.cuda.get_device_name(0), 'faces_per_s': summary}), flush=True)


if __name__ == '__main__':
    main()
