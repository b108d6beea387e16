#!/usr/bin/env python
"""What track clips (KEEP_AMD_TRACK_CLIPS: every clip holds consecutive frames of ONE face track) cost on the MI355X, one call, written as a
text report (default profiles/track_clips.txt).

``process_frames_u8`` end to end (synthetic weights, tools/synth_facehelper.py with the detector resize left to the processor, as with
the reference helper) on multi-face video:
    1080p / 3 faces / 96 frames;   720p / 2 faces / 96 frames
with the knob off -- the parent's path: the flat frame-major crop list cut into clips -- and on, in the same process, warmed, interleaved
round by round, host clock around a synchronise.  Every round is listed, with per call the number of clips the net was handed, the
number of distinct clip lengths (one batch group at least per length), and the time from the start of the call to the first frame
handed to the paste-back (host clock, when its composite is queued): it shows whether the clip order keeps the paste streaming.

The gate, per leg: the best round with the knob on is not slower than the best round with it off by more than the spread between the
off rounds.  A miss is RECORDED (exit status 1), not a reason to drop the mode: it is an opt-in for quality, not a speed mode.  The two
settings restore different clips, so their outputs differ by design; what the mode computes is proved in tests/test_gpu_track_clips.py.

    timeout -k 10 900 python tools/bench_track_clips.py [--rounds 3] [--legs 0,1] [--frames 96] [--out FILE]
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

LEGS = [('1080p, 3 faces', 1080, 1920, 3),
        ('720p, 2 faces', 720, 1280, 2)]


def legs(which, rounds, n, say, flush):
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    from comfyui_keep_amd.engine.paste import GpuPaster
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    seen = {}
    real_run = net.run_clips_u8

    @functools.wraps(real_run)
    def run_clips_u8(clips, *a, **kw):
        seen['lengths'] = [len(c) for c in clips]
        return real_run(clips, *a, **kw)
    net.run_clips_u8 = run_clips_u8
    real_paste = GpuPaster.paste

    def paste(this, *a, **kw):
        seen.setdefault('first', time.perf_counter())
        return real_paste(this, *a, **kw)
    GpuPaster.paste = paste
    ok = True
    for li in which:
        name, H, W, faces = LEGS[li]
        proc, helper = SF.make_processor(net, (H, W), faces)
        helper.resize_for_detector = None                           # the processor resizes the detector inputs, as with the reference helper
        proc.gpu_resize = proc.gpu_detect_resize = True
        g = torch.Generator().manual_seed(li)
        frames = [f.numpy() for f in torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)]

        def run(knob):
            proc.track_clips = knob
            helper.begin_sequence()
            seen.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=20)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert isinstance(res, torch.Tensor) and res.shape[0] == n and proc.frame_store is True
            lengths = seen['lengths']
            return dt, seen['first'] - t0, len(lengths), len(set(lengths))
        say(f"{name}, {n} frames, factor 1.0: {n * H * W * 3 / 1e6:.0f} MB of frames, {n * faces} crops, max_clip_length 20 (seconds per call)")
        run(False)                                                  # warm both forms
        run(True)
        t = {True: [], False: []}
        for _ in range(rounds):
            for knob in (False, True):
                t[knob].append(run(knob))
        off, on = min(r[0] for r in t[False]), min(r[0] for r in t[True])
        spread = max(r[0] for r in t[False]) - off
        leg_ok = on <= off + spread
        ok = ok and leg_ok
        for knob, label in ((False, 'track clips off'), (True, 'track clips on ')):
            best = min(r[0] for r in t[knob])
            say(f"   {label} {[round(r[0], 4) for r in t[knob]]} best {best:.4f} ({n / best:6.1f} frames/s)   {t[knob][0][2]} clips of "
                f"{t[knob][0][3]} distinct length(s);  first frame at the paste-back after {[round(r[1], 4) for r in t[knob]]} s")
        say(f"   on / off {on / off:.3f};  gate on <= off + spread of the off rounds ({spread:.4f} s): {'PASS' if leg_ok else 'MISS'}"
            + ('' if leg_ok else f" by {on - off - spread:.4f} s"))
        flush()
        del proc, helper, frames
        torch.cuda.empty_cache()
    GpuPaster.paste = real_paste
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--legs', default='0,1')
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_clips.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_clips.py measures on the MI355X: no HIP device visible"
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    def say(line=''):
        print(line, flush=True)
        lines.append(line)
    title = f"Track clips (KEEP_AMD_TRACK_CLIPS): one face track per clip in multi-face video, {torch.cuda.get_device_name(0)}"
    say(title)
    say('=' * min(len(title), 140))
    say()
    say(f"Command: python tools/bench_track_clips.py --rounds {a.rounds} --legs {a.legs} --frames {a.frames}   ({time.strftime('%Y-%m-%d')})")
    say("End to end process_frames_u8: host clock around a synchronise, synthetic weights, both settings warmed once, then knob off / knob on")
    say("alternate round by round in one process; knob off is the parent's path.  No counters were collected.  The two settings restore")
    say("different clips, so their outputs differ by design: there is no reference for the mode (the reference never runs its net on one")
    say("track of a multi-face video); tests/test_gpu_track_clips.py proves that every face equals its track restored on its own, bit for bit.")
    say()
    flush()
    ok = legs([int(x) for x in a.legs.split(',') if x != ''], a.rounds, a.frames, say, flush)
    say()
    say(f"GATE over the legs above: {'PASS' if ok else 'MISS (recorded; the mode stays: an opt-in for quality, not a speed mode)'}")
    flush()
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
