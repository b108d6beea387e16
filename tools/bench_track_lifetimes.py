#!/usr/bin/env python
"""What track lifetimes (KEEP_AMD_TRACK_LIFETIMES: a face is restored only while it is seen) change on the MI355X, written as a text
report (default profiles/track_lifetimes.txt).

1. The kernel alone -- ``keep_paste_face_w`` at opacity 1.0 against ``keep_paste_face`` on the 1080p / 3-face paste case
   (engine/synth.py: the three blends of one frame), between device events, the two entries alternating launch by launch, best of the
   launches per round.  The gate: the new entry's best round is not slower than the core entry's by more than the spread of the core
   entry's rounds.  A build without the symbol (the parent commit) skips this part.

2. ``process_frames_u8`` end to end (synthetic weights, tools/synth_facehelper.py with the detector resize left to the processor) on
       1080p / 3 faces / 96 frames
   with scripted detections: face 0 is seen on frames 0-31 only, face 1 on frames 40-71 only, face 2 on every frame but one in every 24
   (frames 12, 36, 60, 84).  The synthetic helper detects every face everywhere, so a wrapper in front of the smoothers drops the rest.
   (Face 1 does not enter on the frame face 0 leaves: with an exit and an entrance on one frame the tracker's cost matrix has a row
   without a finite entry, which scipy's assignment refuses -- the tracker is the reference's and is left as it is.)
   Knob off and knob on, one processor each, warmed, interleaved round by round in one process, best of the rounds, host clock around a
   synchronise.  Per setting: crops restored, clips, frames/s and the time from the start of the call to the first frame handed to the
   paste-back (host clock, when its composite is queued).
   The expectation, stated before the run: the time follows the crop count.  Knob off restores 7 tracks (face 2 is cut into 5 by its
   4 misses) on all 96 frames = 672 crops; knob on 32 + 32 + 96 = 160.

The knob-off cost against the parent commit is measured with tools/bench_track_clips.py, which runs unchanged on both trees.

    timeout -k 10 900 python tools/bench_track_lifetimes.py [--rounds 3] [--frames 96] [--kernel 1] [--e2e 1] [--out FILE]
"""
import argparse
import ctypes as C
import functools
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

CORE, NAME = 'keep_paste_face', 'keep_paste_face_w'
KNOBS = ('KEEP_AMD_TRACK_CLIPS', 'KEEP_AMD_TRACK_CARRY', 'KEEP_AMD_SCENE_CUTS', 'KEEP_AMD_TRACK_LIFETIMES', 'KEEP_AMD_TRACK_MAX_GAP',
         'KEEP_AMD_TRACK_FADE')
SETTINGS = [('knob off', {}), ('track lifetimes', {'KEEP_AMD_TRACK_LIFETIMES': '1'})]


def kernel_alone(say, rounds=3, reps=30):
    from comfyui_keep_amd.engine import hiplib as L
    from comfyui_keep_amd.engine import paste, synth
    if NAME not in getattr(L, '_CV_SIGNATURES', {}):
        say(f"(this build has no {NAME}: the kernel part is skipped)")
        return True
    frame, faces, mats, classes = synth.synth_paste_case()
    H, W = frame.shape[:2]
    gp = paste.GpuPaster('cuda')
    faces_dev = torch.from_numpy(faces).cuda()
    masks = gp.soft_masks(torch.from_numpy(classes).cuda())
    acc0 = torch.from_numpy(frame.astype(np.float32)).cuda()
    acc = acc0.clone()
    d2s = [(C.c_double * 6)(*paste.invert_affine(M).reshape(-1).tolist()) for M in mats]
    boxes = [paste.face_box(M, 512, 512, W, H) for M in mats]
    one = C.c_float(1.0)

    def blends(entry):
        for i in range(len(mats)):
            extra = (one,) if entry == NAME else ()
            L.call(entry, acc, H, W, faces_dev[i], masks[i], 512, 512, d2s[i], *boxes[i], paste.PARSE_BORDER, *extra)

    def timed(entry):
        acc.copy_(acc0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        blends(entry)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    got = {}
    for entry in (CORE, NAME):
        acc.copy_(acc0)
        blends(entry)
        got[entry] = acc.clone()
    assert torch.equal(got[CORE], got[NAME]) and not torch.equal(got[CORE], acc0)
    px = sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in boxes)
    say(f"{NAME} at opacity 1.0 against {CORE}: the 3 blends of the 1080p / 3-face case ({px} box pixels), device events,")
    say(f"the entries alternate launch by launch, either one first in turn, best of {reps} per round after 5 warm ones, {rounds} rounds; the results are bit-identical")
    for _ in range(5):
        timed(CORE), timed(NAME)
    best = {CORE: [], NAME: []}
    for _ in range(rounds):
        t = {CORE: [], NAME: []}
        for r in range(reps):
            for entry in ((CORE, NAME) if r % 2 == 0 else (NAME, CORE)):     # (the second launch of a pair finds the caches warm)
                t[entry].append(timed(entry))
        for entry in t:
            best[entry].append(min(t[entry]))
    for entry in (CORE, NAME):
        say(f"   {entry:18s} {[round(v * 1e6, 2) for v in best[entry]]} us per frame (3 blends), best {min(best[entry]) * 1e6:.2f} us")
    spread = max(best[CORE]) - min(best[CORE])
    ok = min(best[NAME]) <= min(best[CORE]) + spread
    say(f"   new / core {min(best[NAME]) / min(best[CORE]):.3f};  gate new <= core + spread of the core rounds ({spread * 1e6:.2f} us): "
        f"{'PASS' if ok else 'MISS'}")
    return ok


def scripted(t, j):
    """Whether face j is detected on frame t."""
    if j == 0:
        return t < 32
    if j == 1:
        return 40 <= t < 72
    return t % 24 != 12


def end_to_end(rounds, n, say, flush):
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    from comfyui_keep_amd.engine.paste import GpuPaster
    from comfyui_keep_amd.modules import keep_processor as KP
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    seen = {}
    real_run = net.run_clips_u8

    @functools.wraps(real_run)
    def run_clips_u8(clips, *a, **kw):
        seen['clips'], seen['crops'] = len(clips), sum(len(c) for c in clips)
        return real_run(clips, *a, **kw)
    net.run_clips_u8 = run_clips_u8
    real_paste = GpuPaster.paste

    def paste(this, *a, **kw):
        seen.setdefault('first', time.perf_counter())
        return real_paste(this, *a, **kw)
    GpuPaster.paste = paste
    real_smooth = KP.smooth_tracked_faces

    def smooth(raw, *a, **kw):                                      # the scripted detections
        return real_smooth([[lm for j, lm in enumerate(faces) if scripted(t, j)] for t, faces in enumerate(raw)], *a, **kw)
    KP.smooth_tracked_faces = smooth
    H, W, faces = 1080, 1920, 3
    procs = []
    for label, env in SETTINGS:                                     # the knobs are read in the constructor: one processor per setting
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        proc, helper = SF.make_processor(net, (H, W), faces)
        helper.resize_for_detector = None                           # the processor resizes the detector inputs, as with the reference helper
        proc.gpu_resize = proc.gpu_detect_resize = True
        procs.append((label, proc, helper))
    for k in KNOBS:
        os.environ.pop(k, None)
    frames = [f for f in np.random.default_rng(0).integers(0, 256, (n, H, W, 3), dtype=np.uint8)]

    def run(proc, helper):
        helper.begin_sequence()
        seen.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=20)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert isinstance(res, torch.Tensor) and res.shape[0] == n and proc.frame_store is True
        return dt, seen['first'] - t0, seen['crops'], seen['clips'], len(getattr(proc, 'last_track_lifetimes', None) or [])
    detections = sum(scripted(t, j) for t in range(n) for j in range(faces))
    say(f"1080p, 3 faces, {n} frames, factor 1.0, max_clip_length 20: {detections} scripted detections (seconds per call)")
    try:
        for _, proc, helper in procs:
            run(proc, helper)
        t = {label: [] for label, _, _ in procs}
        for _ in range(rounds):
            for label, proc, helper in procs:
                t[label].append(run(proc, helper))
    finally:
        GpuPaster.paste = real_paste
        KP.smooth_tracked_faces = real_smooth
    for label, _, _ in procs:
        rs = [r[0] for r in t[label]]
        _, _, crops, clips, lifetimes = t[label][0]
        say(f"   {label:16s} {[round(v, 4) for v in rs]} best {min(rs):.4f} ({n / min(rs):6.1f} frames/s)  spread {max(rs) - min(rs):.4f}   "
            f"{crops} crops in {clips} clips, {lifetimes} lifetimes;  first frame at the paste-back after {[round(r[1], 4) for r in t[label]]} s")
    off, on = t['knob off'], t['track lifetimes']
    say(f"   on / off: time {min(r[0] for r in on) / min(r[0] for r in off):.3f}, crops {on[0][2] / off[0][2]:.3f}, "
        f"first frame {min(r[1] for r in on) / min(r[1] for r in off):.3f}")
    flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--kernel', type=int, default=1)
    ap.add_argument('--e2e', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_lifetimes.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track_lifetimes.py measures on the MI355X: no HIP device visible"
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    def say(line=''):
        print(line, flush=True)
        lines.append(line)
    title = f"Track lifetimes (KEEP_AMD_TRACK_LIFETIMES): a face is restored only while it is seen, {torch.cuda.get_device_name(0)}"
    say(title)
    say('=' * min(len(title), 140))
    say()
    say(f"Command: python tools/bench_track_lifetimes.py --rounds {a.rounds} --frames {a.frames} --kernel {a.kernel} --e2e {a.e2e}   "
        f"({time.strftime('%Y-%m-%d')})")
    say("No counters were collected.  Not measurable here: the effect on restoration quality with real weights and real video, and whether")
    say("10 frames (KEEP_AMD_TRACK_MAX_GAP) and the tracker's 75 px are good values: both are settings.")
    say()
    ok = True
    if a.kernel:
        ok = kernel_alone(say, a.rounds)
        say()
        flush()
    if a.e2e:
        say("End to end process_frames_u8: host clock around a synchronise, synthetic weights, both settings warmed, then they alternate round")
        say("by round in one process.  Expectation, stated before the run: the time follows the crop count (knob off 672 crops -- 7 tracks, each")
        say("held over all 96 frames --, knob on 160).")
        end_to_end(a.rounds, a.frames, say, flush)
    flush()
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
