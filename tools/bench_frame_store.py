#!/usr/bin/env python
"""The frame store of the detected-sequence path on the MI355X, one call, written as a text report (default profiles/frame_store.txt).

(1) keep_warp_affine_batch_u8 alone: ONE call for 32 faces from 32 resident 1080p frames against 32 keep_warp_affine_u8 launches on
the same frames and maps, device events after warm-up, the two interleaved round by round.  Recorded, not gated.
(2) ``process_frames_u8`` and ``process_image_sequence`` end to end (synthetic weights, tools/synth_facehelper.py with the detector
resize left to the processor, as with the reference helper), KEEP_AMD_FRAME_STORE=1 against KEEP_AMD_FRAME_STORE=0 -- the parent's path
-- in the same process, warmed, interleaved round by round, host clock around a synchronise:
    720p / 1 face / 96 frames;   1080p / 3 faces / 24 frames;   1080p / 1 face / 96 frames at factor 2.0.
Every round is listed.  The gate, per leg and entry point: the store's best round is not slower than the store-off leg's best round by
more than the spread between the store-off leg's own rounds.  Exit status 1 if a leg misses it.

    timeout -k 10 1100 python tools/bench_frame_store.py [--rounds 3] [--legs 0,1,2] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_keep_amd.engine import hiplib as L  # noqa: E402

LEGS = [('720p, 1 face, 96 frames, factor 1.0', 720, 1280, 1, 96, 1.0),
        ('1080p, 3 faces, 24 frames, factor 1.0', 1080, 1920, 3, 24, 1.0),
        ('1080p, 1 face, 96 frames, factor 2.0', 1080, 1920, 1, 96, 2.0)]
BORDER = (135, 133, 132)


def kernel_leg(rounds, reps, say):
    import synth_facehelper as SF
    N = F = 32
    H, W = 1080, 1920
    src = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda')
    out = torch.empty((F, 512, 512, 3), dtype=torch.uint8, device='cuda')
    maps = [SF.track_similarity(t, 0, H, W, 1).reshape(-1).tolist() for t in range(F)]          # crop -> frame IS destination -> source
    idx = (C.c_int32 * F)(*range(F))
    flat = (C.c_double * (6 * F))(*[v for m in maps for v in m])
    each = [(C.c_double * 6)(*m) for m in maps]

    def batched():
        L.call('keep_warp_affine_batch_u8', src, N, H, W, out, F, 512, 512, idx, flat, *BORDER)

    def singles():
        for f in range(F):
            L.call('keep_warp_affine_u8', src[f], H, W, out[f], 512, 512, each[f], *BORDER)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    batched()
    a = out.clone()
    singles()
    torch.cuda.synchronize()
    assert torch.equal(a, out), "the batched call and the single launches disagree"
    legs = {'one batched call': batched, '32 single launches': singles}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    every = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            every[k].append(timed(fn))
    say(f"crop warp of {F} faces (512 x 512) from {N} resident 1080p frames, device events, {rounds} rounds x {reps} repetitions per leg, interleaved (us):")
    for k in legs:
        say(f"   {k:20s} {[round(v, 1) for v in every[k]]}   best {min(every[k]):8.1f} us")
    say(f"   32 single launches / one batched call (best rounds): {min(every['32 single launches']) / min(every['one batched call']):.2f}x; the outputs are bit-equal")


def e2e_legs(which, rounds, say, flush):
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    ok = True
    for li in which:
        name, H, W, faces, n, factor = LEGS[li]
        proc, helper = SF.make_processor(net, (H, W), faces)
        helper.resize_for_detector = None                           # the processor resizes the detector inputs, as with the reference helper
        proc.gpu_resize = proc.gpu_detect_resize = True
        g = torch.Generator().manual_seed(li)
        u8 = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
        frames = [f.numpy() for f in u8]
        comfy = u8.flip(-1).float() / 255.0

        def run(store, entry):
            os.environ['KEEP_AMD_FRAME_STORE'] = '1' if store else '0'
            helper.begin_sequence()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if entry == 'u8':
                res = proc.process_frames_u8(frames, factor, False, False, False, max_clip_length=20)
            else:
                res = proc.process_image_sequence(comfy, factor, False, False, False, max_clip_length=20)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert isinstance(res, torch.Tensor) and res.shape[0] == n and proc.frame_store is True
            return dt, res
        say(f"{name}: {n * H * W * 3 / 1e6:.0f} MB of frames, {n * faces} crops, max_clip_length 20 (seconds per call)")
        for entry in ('u8', 'comfy'):
            label = 'process_frames_u8' if entry == 'u8' else 'process_image_sequence'
            _, a = run(True, entry)                                  # warm both forms; their outputs are the same frames
            _, b = run(False, entry)
            same = torch.equal(a, b)
            del a, b
            t = {True: [], False: []}
            for _ in range(rounds):
                for store in (False, True):
                    t[store].append(run(store, entry)[0])
            off, on = min(t[False]), min(t[True])
            spread = max(t[False]) - min(t[False])
            leg_ok = on <= off + spread
            ok = ok and leg_ok and same
            say(f"   {label:24s} store off {[round(v, 4) for v in t[False]]} best {off:.4f} ({n / off:6.1f} frames/s)")
            say(f"   {'':24s} store on  {[round(v, 4) for v in t[True]]} best {on:.4f} ({n / on:6.1f} frames/s)   on / off {on / off:.3f}")
            say(f"   {'':24s} outputs bit-equal: {same};  gate on <= off + spread of the store-off rounds ({spread:.4f} s): {'PASS' if leg_ok else 'FAIL'}")
            flush()
        del proc, helper, frames, comfy, u8
        torch.cuda.empty_cache()
    os.environ.pop('KEEP_AMD_FRAME_STORE', None)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--legs', default='0,1,2')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frame_store.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frame_store.py measures on the MI355X: no HIP device visible"
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    def say(line=''):
        print(line, flush=True)
        lines.append(line)
    title = f"Frames of a detected sequence resident on the device (KEEP_AMD_FRAME_STORE) and keep_warp_affine_batch_u8, {torch.cuda.get_device_name(0)}"
    say(title)
    say('=' * min(len(title), 140))
    say()
    say(f"Command: python tools/bench_frame_store.py --rounds {a.rounds} --reps {a.reps} --legs {a.legs}   ({time.strftime('%Y-%m-%d')})")
    say("End to end: host clock around a synchronise, synthetic weights, every form warmed once, then store off / store on alternate round by")
    say("round in one process; store off is the parent's path.  No counters were collected.  Not measured here: parity with cv2 itself, and the")
    say("host cv2 path of a ComfyUI installation (the synthetic helper fits similarities in closed form and detects on the engine).")
    say()
    kernel_leg(a.rounds, a.reps, say)
    say()
    flush()
    ok = e2e_legs([int(x) for x in a.legs.split(',') if x != ''], a.rounds, say, flush)
    say()
    say(f"GATE over the legs above: {'PASS' if ok else 'FAIL'}")
    flush()
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
