#!/usr/bin/env python
"""The detection pre-pass of a video (``KEEPFaceProcessor._detect_all``; RetinaFace-R50, synthetic weights, tools/synth_facehelper.py)
with the worker pool taking its share (default) and with the whole pre-pass on the root (KEEP_AMD_POOL_DETECT=0).  One process drives
``--gpus`` ranks; with ``--share-device`` (KEEP_DIST_DEVICE) all of them sit on ONE GPU, and the figures then show what the protocol
costs, not how it scales.  Each setting runs ``--repeats`` times, alternated; the best pass and the per-rank time inside the detector
(``GpuPool.detect_ms_total``: summed by the pool over the windows of that pass) are reported.  Also checks that ``GpuPool.detect`` returns what the root's
``detect_batch`` returns on the same frames, bit for bit.  Prints one JSON object.

    timeout -k 10 600 python tools/bench_pool_detect.py --gpus 3 --share-device [--frames 64 --chunk 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from __graft_entry__ import load_package  # noqa: E402

load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=3)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--chunk', type=int, default=8, help='KEEP_AMD_DETECT_BATCH: frames per detector call')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--share-device', action='store_true', help='every rank on the current device (KEEP_DIST_DEVICE)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pool_detect.py measures on the MI355X: no HIP device visible"
    os.environ['KEEP_AMD_DETECT_BATCH'] = str(a.chunk)
    if a.share_device:
        os.environ['KEEP_DIST_DEVICE'] = str(torch.cuda.current_device())
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    from comfyui_keep_amd.engine.pool import GpuPool
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    H, W = 720, 1280
    proc, helper = SF.make_processor(net, (H, W), 1)
    g = torch.Generator().manual_seed(1)
    frames = [f.numpy() for f in torch.randint(0, 256, (a.frames, H, W, 3), generator=g, dtype=torch.uint8)]
    net.pool = GpuPool(net, a.gpus, timeout=300, join_timeout=120)
    out = {'on': [], 'off': []}
    per_rank = []
    try:
        pool = net.pool
        eng = helper.face_detector.engine
        # what the pool returns against the root alone, on the detector inputs of the first chunks
        _, batch = proc._prep_detect_chunk(frames[:min(a.frames, a.chunk * a.gpus)], 640)
        chunks = [batch[s:s + a.chunk] for s in range(0, len(batch), a.chunk)]
        pool.set_detector(eng)
        got, want = pool.detect(chunks, 0.6), eng.detect_batch(batch, 0.6)
        equal = len(got) == len(want) and all(np.array_equal(x, y) for x, y in zip(got, want))
        n_det = int(sum(len(x) for x in want))
        for rep in range(a.repeats):
            for knob in ('off', 'on'):
                if knob == 'off':
                    os.environ['KEEP_AMD_POOL_DETECT'] = '0'
                else:
                    os.environ.pop('KEEP_AMD_POOL_DETECT', None)
                pool.detect_ms_total.clear()
                helper.begin_sequence()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                raw = proc._detect_all(frames, True)
                torch.cuda.synchronize()
                out[knob].append(round(time.perf_counter() - t0, 4))
                ms = dict(pool.detect_ms_total)                  # (summed by the pool over the windows of this pass)
                assert len(raw) == a.frames and (knob == 'on') == bool(ms)
                if knob == 'on':
                    per_rank.append({str(r): round(v, 1) for r, v in sorted(ms.items())})
    finally:
        net.pool.close()
        net.pool = None
    best = out['on'].index(min(out['on']))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "ranks": a.gpus, "ranks_share_one_device": bool(a.share_device),
                      "frame_size": [H, W], "frames": a.frames, "frames_per_chunk": a.chunk, "detector": "retinaface_resnet50 x3",
                      "pool_detect_equals_root_detect_batch": equal, "detections_compared": n_det,
                      "prepass_seconds": {"KEEP_AMD_POOL_DETECT=0": out['off'], "unset": out['on']},
                      "detect_ms_per_rank_best_pass": per_rank[best]}), flush=True)
    assert equal


if __name__ == '__main__':
    main()
