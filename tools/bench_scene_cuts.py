#!/usr/bin/env python
"""What scene cuts (KEEP_AMD_SCENE_CUTS: tracks, smoothing and the carried state stop at hard cuts) cost on the MI355X, written as a text
report (default profiles/scene_cuts.txt).

1. The kernel alone -- ``keep_frame_signature_u8``, 32 frames per launch at 720p, 1080p and 2160p, on noise frames and on flat-colour
   frames (every pixel of a cell in ONE bin: the worst case of a histogram) -- between device events, best of the repeats, as
   microseconds per frame and as the fraction of the 8 TB/s HBM peak its input bytes make.  A build without the symbol (the parent
   commit) skips this part.

2. ``process_frames_u8`` end to end (synthetic weights, tools/synth_facehelper.py with the detector resize left to the processor) on
       720p / 1 face / 96 frames;   1080p / 3 faces / 96 frames
   over a cut-free video (noise) and one with a hard cut every 24 frames (dark noise / bright noise scenes), in three settings --
   knob off, track clips, track clips + scene cuts -- one processor each, warmed, interleaved round by round, best of the rounds, host
   clock around a synchronise.  The settings are made with environment variables ONLY, so this file runs unchanged on the parent
   commit, which ignores the new one: ``--json FILE`` writes the timings, ``--parent-json FILE`` reads the parent's and prints the gate:
     * knob off: this commit is not slower than the parent by more than the spread of the parent's rounds;
     * cut-free video: the scene-cuts setting is not slower than the PARENT's track-clips setting by more than that spread.
   The with-cuts video is reported, not gated: more and shorter clips cost what they cost.

    timeout -k 10 900 python tools/bench_scene_cuts.py [--rounds 3] [--legs 0,1] [--frames 96] [--kernel 1] [--out FILE]
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

LEGS = [('720p, 1 face', 720, 1280, 1),
        ('1080p, 3 faces', 1080, 1920, 3)]
SETTINGS = [('knob off', {}),
            ('track clips', {'KEEP_AMD_TRACK_CLIPS': '1'}),
            ('track clips + scene cuts', {'KEEP_AMD_TRACK_CLIPS': '1', 'KEEP_AMD_SCENE_CUTS': '1'})]
KNOBS = ('KEEP_AMD_TRACK_CLIPS', 'KEEP_AMD_TRACK_CARRY', 'KEEP_AMD_SCENE_CUTS', 'KEEP_AMD_SCENE_CUT_THRESHOLD')
HBM_PEAK = 8.0e12
NAME = 'keep_frame_signature_u8'


def kernel_alone(say, reps=20):
    from comfyui_keep_amd.engine import hiplib as L
    if NAME not in getattr(L, '_CV_SIGNATURES', {}):
        say(f"(this build has no {NAME}: the kernel part is skipped)")
        return
    say(f"{NAME} alone: 32 frames per launch, device events, best of {reps} launches after 3 warm ones")
    say("   (the zero-fill of the counters is part of the call and of the time)")
    N = 32
    for label, H, W in (('720p', 720, 1280), ('1080p', 1080, 1920), ('2160p', 2160, 3840)):
        for content in ('noise', 'flat'):
            if content == 'noise':
                frames = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device='cuda')
            else:
                frames = torch.full((N, H, W, 3), 200, dtype=torch.uint8, device='cuda')
            sig = torch.empty((N, 256), dtype=torch.int32, device='cuda')
            for _ in range(3):
                L.call(NAME, frames, N, H, W, sig)
            torch.cuda.synchronize()
            assert bool((sig.sum(dim=1) == H * W).all())
            best = float('inf')
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.call(NAME, frames, N, H, W, sig)
                e1.record()
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1) * 1e-3)
            per = best / N
            say(f"   {label:5s} {content:5s}  {per * 1e6:7.2f} us per frame   {H * W * 3 / per / 1e12:5.2f} TB/s of input   "
                f"{H * W * 3 / per / HBM_PEAK:4.2f} of the 8 TB/s peak")
            del frames, sig
            torch.cuda.empty_cache()


def video(kind, n, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == 'cut-free':
        return [f for f in rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)]
    out = []
    for s, a in enumerate(range(0, n, 24)):                         # a hard cut every 24 frames: dark noise / bright noise
        lo, hi = ((0, 128), (128, 256))[s % 2]
        out.extend(f for f in rng.integers(lo, hi, (min(24, n - a), H, W, 3), dtype=np.uint8))
    return out


def end_to_end(which, rounds, n, say, flush, results):
    import functools
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    seen = {}
    real_run = net.run_clips_u8

    @functools.wraps(real_run)
    def run_clips_u8(clips, *a, **kw):
        seen['clips'] = len(clips)
        return real_run(clips, *a, **kw)
    net.run_clips_u8 = run_clips_u8
    for li in which:
        name, H, W, faces = LEGS[li]
        procs = []
        for label, env in SETTINGS:                                 # the knobs are read in the constructor: one processor per setting
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            proc, helper = SF.make_processor(net, (H, W), faces)
            helper.resize_for_detector = None                       # the processor resizes the detector inputs, as with the reference helper
            proc.gpu_resize = proc.gpu_detect_resize = True
            procs.append((label, proc, helper))
        for k in KNOBS:
            os.environ.pop(k, None)
        for kind in ('cut-free', 'a cut every 24 frames'):
            frames = video(kind, n, H, W, li)

            def run(proc, helper):
                helper.begin_sequence()
                seen.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=20)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert isinstance(res, torch.Tensor) and res.shape[0] == n and proc.frame_store is True
                return dt, seen['clips'], len(getattr(proc, 'last_scene_cuts', None) or [])
            say(f"{name}, {n} frames, {kind}, factor 1.0: {n * faces} crops, max_clip_length 20 (seconds per call)")
            for _, proc, helper in procs:
                run(proc, helper)
            t = {label: [] for label, _, _ in procs}
            for _ in range(rounds):
                for label, proc, helper in procs:
                    t[label].append(run(proc, helper))
            for label, _, _ in procs:
                rs = [r[0] for r in t[label]]
                say(f"   {label:25s} {[round(v, 4) for v in rs]} best {min(rs):.4f} ({n / min(rs):6.1f} frames/s)  spread {max(rs) - min(rs):.4f}   "
                    f"{t[label][0][1]} clips, {t[label][0][2]} cuts found")
                results[f"{name} | {kind} | {label}"] = rs
            flush()
            del frames
        del procs
        torch.cuda.empty_cache()


def gate(say, results, parent):
    say()
    say("Against the parent commit (the same file, run on the parent's tree on the same box just before; it ignores KEEP_AMD_SCENE_CUTS)")
    say("---------------------------------------------------------------------------------------------------------------------------")
    ok = True
    for key in sorted(results):
        leg, kind, label = key.split(' | ')
        if label == 'knob off':
            base = parent.get(key)
        elif label == 'track clips + scene cuts' and kind == 'cut-free':
            base = parent.get(f"{leg} | {kind} | track clips")
        else:
            continue
        if not base:
            continue
        spread, pb, tb = max(base) - min(base), min(base), min(results[key])
        verdict = 'PASS' if tb <= pb + spread else 'MISS'
        gated = label == 'knob off' or kind == 'cut-free'
        ok = ok and (verdict == 'PASS' or not gated)
        against = 'knob off' if label == 'knob off' else 'track clips'
        say(f"{leg:15s} {kind:22s} {label:25s} {tb:.4f} s   parent's {against} {pb:.4f} s (spread of its rounds {spread:.4f} s)   "
            f"this / parent {tb / pb:.3f}   {verdict}")
    say(f"Condition over the gated rows: {'PASS' if ok else 'MISS'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--legs', default='0,1')
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--kernel', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_cuts.txt'))
    ap.add_argument('--json', default=None)
    ap.add_argument('--parent-json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scene_cuts.py measures on the MI355X: no HIP device visible"
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    def say(line=''):
        print(line, flush=True)
        lines.append(line)
    title = f"Scene cuts (KEEP_AMD_SCENE_CUTS): tracks, smoothing and carry stop at hard cuts, {torch.cuda.get_device_name(0)}"
    say(title)
    say('=' * min(len(title), 140))
    say()
    say(f"Command: python tools/bench_scene_cuts.py --rounds {a.rounds} --legs {a.legs} --frames {a.frames} --kernel {a.kernel}   "
        f"({time.strftime('%Y-%m-%d')})")
    say("No counters were collected.  Not measurable here: the default threshold's behaviour on real video (flashes, dissolves, fast pans)")
    say("and the effect on restoration quality with real weights.")
    say()
    if a.kernel:
        kernel_alone(say)
        say()
        flush()
    say("End to end process_frames_u8: host clock around a synchronise, synthetic weights, every setting warmed, then the settings")
    say("alternate round by round in one process.")
    results = {}
    end_to_end([int(x) for x in a.legs.split(',') if x != ''], a.rounds, a.frames, say, flush, results)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
    if a.parent_json:
        with open(a.parent_json) as f:
            gate(say, results, json.load(f))
    flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
