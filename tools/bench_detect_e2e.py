#!/usr/bin/env python
"""``KEEPFaceProcessor.process_frames_u8`` end to end (detect, crop, restore, parse, paste; synthetic weights, tools/synth_facehelper.py)
at 720p / 1 face under both settings of KEEP_AMD_DETECT_PRECISION: x3 (default) and f16 (RetinaFace-R50).  One process; each setting runs
twice, alternated, and the second pass is reported.  Prints one JSON object.

    timeout -k 10 600 python tools/bench_detect_e2e.py [--frames 24]
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
from comfyui_keep_amd.engine import retinaface as RF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=24)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_detect_e2e.py measures on the MI355X: no HIP device visible"
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    H, W, faces = 720, 1280, 1
    proc, helper = SF.make_processor(net, (H, W), faces)
    weights = RF.synth_retinaface_state_dict(seed=0)
    detectors = {p: RF.EngineRetinaFace(RF.RetinaFaceEngine(weights, precision=p).to(dev)) for p in ('x3', 'f16')}
    g = torch.Generator().manual_seed(faces)
    frames = [f.numpy() for f in torch.randint(0, 256, (a.frames, H, W, 3), generator=g, dtype=torch.uint8)]
    out = {}
    for prec in ('x3', 'f16', 'x3', 'f16'):
        helper.face_detector = detectors[prec]
        helper.begin_sequence()
        t0 = time.perf_counter()
        res = proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=20)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert tuple(res.shape) == (a.frames, H, W, 3)
        out[prec] = {"frames_per_s": round(a.frames / dt, 2), "seconds": round(dt, 3), "frames": a.frames}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "frame_size": [H, W], "faces_per_frame": faces,
                      "entry_point": "KEEPFaceProcessor.process_frames_u8", "KEEP_AMD_DETECT_PRECISION": out}), flush=True)


if __name__ == '__main__':
    main()
