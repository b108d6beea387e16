#!/usr/bin/env python
"""Small frames (short side below 512) on the device path on the MI355X, one call, written as a text report (default
profiles/small_frames.txt).

``process_frames_u8`` and ``process_image_sequence`` end to end (synthetic weights, tools/synth_facehelper.py) over 96 frames of
480 x 854 with 1 face, with a helper whose ``read_image`` enlarges every frame to a short side of 512 as
face_restoration_helper.py:182-184 does.  KEEP_AMD_GPU_SMALL_FRAMES on -- the frame store keeps the sequence, one
keep_resize_linear_fxy_u8 launch per chunk, ``read_image`` once -- against off -- ``read_image`` twice per frame, three uploads per frame,
one warp launch per face, the backgrounds resized on the paste stream -- in the same process, warmed, interleaved round by round, host
clock around a synchronise.  Every round is listed.

The stand-in helper has no cv2: its ``read_image`` enlarges on the HOST with ``torch.nn.functional.interpolate(mode='bilinear')`` (the
threads torch is given), which is OTHER ARITHMETIC than cv2.resize's fixed point and costs what it costs, not what cv2 costs: the off leg
is a stand-in for a ComfyUI installation's, whose host cv2 path is not measured here.  (The numpy restatement of cv2.resize in tests/
is an order of magnitude slower than either and would flatter the device path.)  Because the two legs enlarge with different arithmetic
their outputs are not compared here; tests/test_gpu_small_frames.py holds both paths to the same bits.

The gate is the frame store's own, per entry point: the on leg's best round is not slower than the off leg's best round by more than the
spread between the off leg's own rounds.  Exit status 1 if an entry point misses it.

    timeout -k 10 600 python tools/bench_small_frames.py [--rounds 3] [--frames 96] [--out FILE]
"""
import argparse
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

H, W, FACES = 480, 854, 1


def helper_class():
    import synth_facehelper as SF
    from comfyui_keep_amd.engine.resize import LinearResizer

    class HostBilinearHelper(SF.SynthFaceHelper):
        reads = 0

        def read_image(self, img):
            self.reads += 1
            self.input_img, self.is_gray = img, False
            h, w = img.shape[:2]
            if min(h, w) < 512:
                f = 512.0 / min(h, w)
                w2, h2 = LinearResizer.enlarged_size(h, w, f, f)
                x = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)[None].float()
                y = torch.nn.functional.interpolate(x, size=(h2, w2), mode='bilinear', align_corners=False)
                self.input_img = y.round_().clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous().numpy()
    return HostBilinearHelper


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'small_frames.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_small_frames.py measures on the MI355X: no HIP device visible"
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    from comfyui_keep_amd.engine.resize import LinearResizer
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    def say(line=''):
        print(line, flush=True)
        lines.append(line)
    n = a.frames
    f = 512.0 / min(H, W)
    W2, H2 = LinearResizer.enlarged_size(H, W, f, f)
    title = f"Small frames on the device path (KEEP_AMD_GPU_SMALL_FRAMES), {torch.cuda.get_device_name(0)}"
    say(title)
    say('=' * len(title))
    say()
    say(f"Command: python tools/bench_small_frames.py --rounds {a.rounds} --frames {n}   ({time.strftime('%Y-%m-%d')})")
    say("End to end: host clock around a synchronise, synthetic weights, both forms warmed once, then off / on alternate round by round in")
    say("one process.  The helper's read_image enlarges on the host with F.interpolate(mode='bilinear'): OTHER ARITHMETIC than cv2.resize's,")
    say(f"on {torch.get_num_threads()} host threads; off is the parent's path over that stand-in.  No counters were collected.  Not measured")
    say("here: parity with cv2 itself, and the host cv2 path of a ComfyUI installation.")
    say()
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    proc, helper = SF.make_processor(net, (H2, W2), FACES)                 # (the track geometry lives in the enlarged frame)
    helper.__class__ = helper_class()
    proc.gpu_resize = proc.gpu_detect_resize = True
    u8 = torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    frames = [fr.numpy() for fr in u8]
    comfy = u8.flip(-1).float() / 255.0

    def run(on, entry):
        proc.gpu_small_frames = bool(on)
        helper.begin_sequence()
        helper.reads = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if entry == 'u8':
            res = proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=20)
        else:
            res = proc.process_image_sequence(comfy, 1.0, False, False, False, max_clip_length=20)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert isinstance(res, torch.Tensor) and tuple(res.shape) == (n, H2, W2, 3) and proc.frame_store is True
        assert helper.reads == (1 if on else 2 * n), helper.reads       # the path under test really ran
        return dt
    say(f"{H} x {W} -> {H2} x {W2}, {FACES} face, {n} frames, factor 1.0: {n * H * W * 3 / 1e6:.0f} MB of frames, {n * FACES} crops, "
        f"max_clip_length 20 (seconds per call)")
    ok = True
    for entry in ('u8', 'comfy'):
        label = 'process_frames_u8' if entry == 'u8' else 'process_image_sequence'
        run(True, entry)
        run(False, entry)
        t = {True: [], False: []}
        for _ in range(a.rounds):
            for on in (False, True):
                t[on].append(run(on, entry))
        off, best = min(t[False]), min(t[True])
        spread = max(t[False]) - min(t[False])
        leg_ok = best <= off + spread
        ok = ok and leg_ok
        say(f"   {label:24s} path off {[round(v, 4) for v in t[False]]} best {off:.4f} ({n / off:6.1f} frames/s)")
        say(f"   {'':24s} path on  {[round(v, 4) for v in t[True]]} best {best:.4f} ({n / best:6.1f} frames/s)   on / off {best / off:.3f}")
        say(f"   {'':24s} gate on <= off + spread of the off rounds ({spread:.4f} s): {'PASS' if leg_ok else 'FAIL'}")
        flush()
    say()
    say(f"GATE over the entry points above: {'PASS' if ok else 'FAIL'}")
    flush()
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
