#!/usr/bin/env python
"""final_upscale_factor on the MI355X: (1) keep_resize_lanczos4_u8 alone, timed with device events after warm-up -- us per frame and
achieved bytes/s = (input + output bytes) / time against the 8 TB/s HBM peak, N = 1 and 16 frames per launch, at 1080p -> 2160p,
720p -> 1440p and 1080p -> 540p; (2) ``process_frames_u8`` end to end (synthetic weights, tools/synth_facehelper.py) at 1080p with 3
faces, factors 1.0 and 2.0.  Prints one JSON object.

    python tools/bench_resize.py [--frames 24] [--skip-e2e]
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
from comfyui_keep_amd.engine.resize import Lanczos4Resizer  # noqa: E402

HBM_PEAK = 8.0e12


def kernel_leg(reps=50):
    rz = Lanczos4Resizer('cuda')
    rows = []
    for (H, W), (H2, W2) in (((1080, 1920), (2160, 3840)), ((720, 1280), (1440, 2560)), ((1080, 1920), (540, 960))):
        for N in (1, 16):
            x = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda')
            for _ in range(5):
                rz.resize_u8(x, W2, H2)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                rz.resize_u8(x, W2, H2)
            e1.record()
            torch.cuda.synchronize()
            s = e0.elapsed_time(e1) / 1e3 / reps
            nbytes = N * 3 * (H * W + H2 * W2)
            rows.append({"src": [H, W], "dst": [H2, W2], "N": N, "us_per_launch": round(s * 1e6, 1),
                         "us_per_frame": round(s * 1e6 / N, 1), "bytes_per_s": round(nbytes / s / 1e12, 3),
                         "unit_bytes_per_s": "TB/s", "fraction_of_hbm_peak": round(nbytes / s / HBM_PEAK, 3)})
    return rows


def e2e_leg(n_frames):
    import synth_facehelper as SF
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.net import KeepNet
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(torch.device('cuda', torch.cuda.current_device())).eval()
    H, W, faces = 1080, 1920, 3
    proc, helper = SF.make_processor(net, (H, W), faces)
    g = torch.Generator().manual_seed(faces)
    frames = [f.numpy() for f in torch.randint(0, 256, (n_frames, H, W, 3), generator=g, dtype=torch.uint8)]
    out = {}
    for factor in (1.0, 2.0, 1.0, 2.0):              # (alternated: the second pass of each is the one reported)
        helper.begin_sequence()
        t0 = time.perf_counter()
        res = proc.process_frames_u8(frames, factor, False, False, False, max_clip_length=20)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert tuple(res.shape) == (n_frames, int(H * factor), int(W * factor), 3)
        out[str(factor)] = {"frames_per_s": round(n_frames / dt, 2), "seconds": round(dt, 3), "frames": n_frames}
    return {"frame_size": [H, W], "faces_per_frame": faces, "entry_point": "KEEPFaceProcessor.process_frames_u8", "factors": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=24)
    ap.add_argument('--skip-e2e', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resize.py measures on the MI355X: no HIP device visible"
    rec = {"device": torch.cuda.get_device_name(0), "kernel": kernel_leg()}
    print(json.dumps(rec), flush=True)
    if not a.skip_e2e:
        rec["process_frames_u8"] = e2e_leg(a.frames)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
