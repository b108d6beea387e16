#!/usr/bin/env python
"""The detector-input resize on the MI355X.  (1) keep_resize_area_u8 alone (engine/resize.py:AreaResizer), timed with device events after
warm-up: us per frame and achieved bytes/s = (input + output bytes) / time against the 8 TB/s HBM peak, 32 frames per launch at
1080p, 720p and 2160p -> 640 x 1137, interleaved round by round with the only other device-side resize there is without cv2 --
``F.interpolate(mode='area')`` + round + cast, what tools/synth_facehelper.py's stand-in does (other arithmetic than cv2's).  (2) With
--e2e: ``process_frames_u8`` end to end (synthetic weights) at 1080p / 1 face with the stand-in's own resize and with a helper that
brings none (KEEP_AMD_GPU_DETECT_RESIZE on: one keep_resize_area_u8 launch per detector chunk), alternated, second pass reported.
Prints one JSON object.

    timeout -k 10 600 python tools/bench_detect_resize.py [--rounds 5] [--reps 20] [--e2e] [--frames 24]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_keep_amd.engine.resize import AreaResizer  # noqa: E402

HBM_PEAK = 8.0e12
N = 32
H2, W2 = 640, 1137


def torch_area(x):
    y = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2).float(), size=(H2, W2), mode='area')
    return y.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def kernel_leg(rounds, reps):
    rz = AreaResizer('cuda')
    rows = []
    for H, W in ((1080, 1920), (720, 1280), (2160, 3840)):
        x = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda')
        legs = {'keep_resize_area_u8': lambda: rz.resize_u8(x, W2, H2), 'torch_interpolate_area': lambda: torch_area(x)}
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        best = {k: float('inf') for k in legs}
        every = {k: [] for k in legs}
        for _ in range(rounds):                                   # interleaved: both see the same neighbours on the machine
            for k, fn in legs.items():
                s = timed(fn, reps)
                every[k].append(round(s * 1e6 / N, 2))
                best[k] = min(best[k], s)
        nbytes = N * 3 * (H * W + H2 * W2)
        row = {"src": [H, W], "dst": [H2, W2], "frames_per_launch": N, "input_plus_output_bytes": nbytes}
        for k in legs:
            row[k] = {"us_per_frame_best": round(best[k] * 1e6 / N, 2), "us_per_frame_rounds": every[k],
                      "GB_per_s": round(nbytes / best[k] / 1e9, 1), "fraction_of_hbm_peak": round(nbytes / best[k] / HBM_PEAK, 4)}
        diff = (rz.resize_u8(x[:1], W2, H2).int() - torch_area(x[:1]).int()).abs()
        row["stand_in_vs_kernel"] = {"max_abs_diff": int(diff.max()), "fraction_differing": round(float((diff > 0).float().mean()), 4)}
        rows.append(row)
        del x
    return rows


def e2e_leg(n_frames):
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    H, W, faces = 1080, 1920, 1
    proc, helper = SF.make_processor(net, (H, W), faces)
    proc.gpu_detect_resize = True                                  # (KEEP_AMD_GPU_DETECT_RESIZE=1)
    g = torch.Generator().manual_seed(faces)
    frames = [f.numpy() for f in torch.randint(0, 256, (n_frames, H, W, 3), generator=g, dtype=torch.uint8)]
    launches = []
    from comfyui_keep_amd.engine import hiplib as L
    real = L.call
    L.call = lambda name, *a: (launches.append(name) if name == 'keep_resize_area_u8' else None, real(name, *a))[1]
    out = {}
    for leg in ('helper_stand_in', 'device_area', 'helper_stand_in', 'device_area'):
        if leg == 'device_area':
            helper.resize_for_detector = None                      # a helper without a resize of its own
        else:
            helper.__dict__.pop('resize_for_detector', None)
        helper.begin_sequence()
        launches.clear()
        t0 = time.perf_counter()
        res = proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=20)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert tuple(res.shape) == (n_frames, H, W, 3)
        assert (len(launches) > 0) == (leg == 'device_area') and proc.gpu_detect_resize is True
        out[leg] = {"frames_per_s": round(n_frames / dt, 2), "seconds": round(dt, 3), "frames": n_frames,
                    "keep_resize_area_u8_launches": len(launches)}
    L.call = real
    return {"frame_size": [H, W], "faces_per_frame": faces, "entry_point": "KEEPFaceProcessor.process_frames_u8", "detector_resize": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--e2e', action='store_true')
    ap.add_argument('--frames', type=int, default=24)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_detect_resize.py measures on the MI355X: no HIP device visible"
    rec = {"device": torch.cuda.get_device_name(0), "kernel": kernel_leg(a.rounds, a.reps)}
    print(json.dumps(rec), flush=True)
    if a.e2e:
        rec["process_frames_u8"] = e2e_leg(a.frames)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
