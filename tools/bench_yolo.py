"""YOLOv5-face on the engine: frames/s of ``yolo_detect_batch`` under the 'x3' and 'f16' policies, and the per-launch-shape A/B of the two.

One process, synthetic weights, uint8 frames from the host (what the processor's pre-pass hands over).  Per (model, size, policy):
WARMUP calls, then REPS timed calls -- wall clock around the call, which ends with its own device-to-host copy -- and the median is
reported.  Then every keep_conv2d launch of one forward is bracketed by HIP events (``Ops.profile``) under
both policies and the launches are grouped by shape: the table shows which kernel each policy plans for a shape and the median time of its
launches, 1x1 shapes first.  A shape whose f16 time exceeds its x3 time is marked SLOWER.  Prints one JSON line per measurement and a
closing summary line.  Run every invocation under a time limit of its own, e.g. ``timeout -k 10 600 python tools/bench_yolo.py``."""
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
from comfyui_keep_amd.engine import yoloface as YF  # noqa: E402

SIZES = {'720p': (720, 1280), '1080p': (1080, 1920)}


def shape_times(eng, x, reps):
    """shape -> (kernel, launches per forward, median over ``reps`` forwards of the summed event time of the shape's launches, ms)."""
    per = {}
    for _ in range(reps):
        eng.o.profile = []
        eng.forward_nhwc(x)
        torch.cuda.synchronize()
        acc = {}
        for kernel, _, split, e0, e1, _, shape in eng.o.profile:
            k = shape[1:]                                       # (H, W, Cin, Cout, KH, stride, upsample, prologue)
            t = acc.setdefault(k, [kernel, 0, 0.0])
            t[1] += 1
            t[2] += e0.elapsed_time(e1)
        eng.o.profile = None
        for k, (kernel, n, ms) in acc.items():
            per.setdefault(k, (kernel, n, []))[2].append(ms)
    return {k: (kernel, n, statistics.median(ms)) for k, (kernel, n, ms) in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=['YOLOv5l', 'YOLOv5n'])
    ap.add_argument('--sizes', nargs='+', default=['720p', '1080p'], choices=list(SIZES))
    ap.add_argument('--precisions', nargs='+', default=['x3', 'f16'])
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--ab-reps', type=int, default=5, help='forwards per policy for the per-shape table (0: no table)')
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    summary, slower = {}, []
    import types
    for bb in a.models:
        W = YF.synth_yolo_state_dict(bb, seed=0)
        engines = {p: YF.YoloFaceEngine(W, precision=p).to('cuda') for p in a.precisions}
        dets = {p: types.SimpleNamespace(detector=YF.EngineYoloModel(e), target_size=None, min_face=10, device='cuda') for p, e in engines.items()}
        for size in a.sizes:
            H, Wd = SIZES[size]
            frames = torch.randint(0, 256, (a.frames, H, Wd, 3), generator=g, dtype=torch.uint8)
            for prec, eng in engines.items():
                for _ in range(a.warmup):
                    YF.yolo_detect_batch(dets[prec], frames)
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    YF.yolo_detect_batch(dets[prec], frames)
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                med = statistics.median(ms)
                rec = {'model': bb, 'size': size, 'precision': prec, 'frames': a.frames, 'median_ms': round(med, 3), 'min_ms': round(min(ms), 3),
                       'max_ms': round(max(ms), 3), 'frames_per_s': round(a.frames / med * 1e3, 1), 'reps': a.reps}
                summary[f'{bb}_{size}_{prec}'] = rec['frames_per_s']
                print(json.dumps(rec), flush=True)
            if a.ab_reps > 0 and {'x3', 'f16'} <= set(engines):
                (rh, rw), (top, left), (H2, W2) = YF.letterbox_geometry(H, Wd)
                x = torch.empty((a.frames, H2, W2, 3), dtype=torch.float32, device='cuda')
                L.call('keep_yolo_letterbox_u8', frames.cuda(), x, a.frames, H, Wd, rh, rw, top, left, H2, W2, 1)
                tab = {p: shape_times(engines[p], x, a.ab_reps) for p in ('x3', 'f16')}
                print(f'# {bb} {size} ({H2} x {W2} letterbox) x {a.frames} frames: per launch shape (H W Cin Cout k stride), launches per forward, ms per forward of the shape', flush=True)
                for k in sorted(tab['x3'], key=lambda k: (k[4] != 1, -tab['x3'][k][2])):
                    k3, n, t3 = tab['x3'][k]
                    k16, _, t16 = tab['f16'][k]
                    mark = '' if k16 == k3 else ('  SLOWER' if t16 > t3 else f'  x{t3 / t16:.2f}')
                    if k16 != k3 and t16 > t3:
                        slower.append({'model': bb, 'size': size, 'shape': k[:6], 'x3_ms': round(t3, 4), 'f16_ms': round(t16, 4)})
                    print(f'{k[0]:5d} {k[1]:5d} {k[2]:5d} {k[3]:5d} {k[4]} {k[5]}  n={n:2d}  x3 {t3:8.3f} [{k3}]  f16 {t16:8.3f} [{k16}]{mark}', flush=True)
                print(json.dumps({'ab': f'{bb} {size}', 'conv_ms_x3': round(sum(v[2] for v in tab['x3'].values()), 3),
                                  'conv_ms_f16': round(sum(v[2] for v in tab['f16'].values()), 3)}), flush=True)
            del frames
        del engines
    print(json.dumps({'bench': 'yolo_detect_batch', 'device': torch.cuda.get_device_name(0), 'frames_per_s': summary, 'slower_shapes': slower}), flush=True)


if __name__ == '__main__':
    main()
