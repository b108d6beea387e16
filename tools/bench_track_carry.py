#!/usr/bin/env python
"""What carried clips (KEEP_AMD_TRACK_CARRY: a clip that continues a face track starts from the state its predecessor left) cost on the
MI355X, one call, written as a text report (default profiles/track_carry.txt).

``process_frames_u8`` end to end (synthetic weights, tools/synth_facehelper.py with the detector resize left to the processor, as with
the reference helper) on
    720p / 1 face / 96 frames;   1080p / 3 faces / 96 frames
with the knob off -- the parent's path: every clip restored from nothing, all clips of a length in one call -- and on, in the same
process, warmed, interleaved round by round, best of the rounds, host clock around a synchronise.  Every round is listed, with per
call the number of clips and how many of them continue another.

No speed is fixed for the knob-on setting: a track's clips now run one after the other (a single-face video has ONE clip in flight,
a three-face video three), and a call that takes or returns a state runs eagerly -- it is never captured into a hipGraph --, so it is
expected near the one-clip eager rate.  The ratio and the frames/s are reported.  The two settings
restore different frames by design; what the mode computes is proved in tests/test_gpu_track_carry.py.

    timeout -k 10 900 python tools/bench_track_carry.py [--rounds 3] [--legs 0,1] [--frames 96] [--out FILE]
"""
import argparse
import functools
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from __graft_entry__ import load_package  # noqa: E402

load_package()

LEGS = [('720p, 1 face', 720, 1280, 1),
        ('1080p, 3 faces', 1080, 1920, 3)]


def legs(which, rounds, n, say, flush):
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
        seen['carried'] = sum(p is not None for p in (kw.get('after') or []))
        return real_run(clips, *a, **kw)
    net.run_clips_u8 = run_clips_u8
    for li in which:
        name, H, W, faces = LEGS[li]
        proc, helper = SF.make_processor(net, (H, W), faces)
        helper.resize_for_detector = None                           # the processor resizes the detector inputs, as with the reference helper
        proc.gpu_resize = proc.gpu_detect_resize = True
        g = torch.Generator().manual_seed(li)
        frames = [f.numpy() for f in torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)]

        def run(knob):
            proc.track_carry = knob
            helper.begin_sequence()
            seen.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=20)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert isinstance(res, torch.Tensor) and res.shape[0] == n and proc.frame_store is True
            return dt, seen['clips'], seen['carried']
        say(f"{name}, {n} frames, factor 1.0: {n * faces} crops, max_clip_length 20 (seconds per call)")
        run(False)                                                  # warm both forms
        run(True)
        t = {True: [], False: []}
        for _ in range(rounds):
            for knob in (False, True):
                t[knob].append(run(knob))
        off, on = min(r[0] for r in t[False]), min(r[0] for r in t[True])
        for knob, label in ((False, 'carry off'), (True, 'carry on ')):
            best = min(r[0] for r in t[knob])
            say(f"   {label} {[round(r[0], 4) for r in t[knob]]} best {best:.4f} ({n / best:6.1f} frames/s)   {t[knob][0][1]} clips, "
                f"{t[knob][0][2]} of them carried")
        say(f"   on / off {on / off:.3f}   (spread of the off rounds {max(r[0] for r in t[False]) - off:.4f} s)")
        flush()
        del proc, helper, frames
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--legs', default='0,1')
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_carry.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_carry.py measures on the MI355X: no HIP device visible"
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    def say(line=''):
        print(line, flush=True)
        lines.append(line)
    title = f"Carried clips (KEEP_AMD_TRACK_CARRY): a track's clips continue one another, {torch.cuda.get_device_name(0)}"
    say(title)
    say('=' * min(len(title), 140))
    say()
    say(f"Command: python tools/bench_track_carry.py --rounds {a.rounds} --legs {a.legs} --frames {a.frames}   ({time.strftime('%Y-%m-%d')})")
    say("End to end process_frames_u8: host clock around a synchronise, synthetic weights, both settings warmed, then knob off / knob on")
    say("alternate round by round in one process; knob off is the parent's path.  No counters were collected.  No speed is fixed for the")
    say("knob-on setting: the clips of a track run one after the other, so a single-face video has one clip in flight.  The two settings")
    say("restore different frames by design; tests/test_gpu_track_carry.py proves what the mode computes.")
    say()
    flush()
    legs([int(x) for x in a.legs.split(',') if x != ''], a.rounds, a.frames, say, flush)
    flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
