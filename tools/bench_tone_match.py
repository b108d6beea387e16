#!/usr/bin/env python
"""What the tone match kernel (``keep_tone_match_u8``: restored faces keep the source crop's low band) takes on the MI355X, written as a
text report (default profiles/tone_match.txt).

The kernel alone at 1, 3 and 32 faces of 512 x 512 and sigma 4, 16 and 40 (R = 12, 48, 120) on noise, between device events, every
round written down, as microseconds per face and as the fraction of the 8 TB/s HBM peak of the bytes that must move: 3 x 786,432 per face
(src and rst read, out written) without the int16 intermediate, 6 x with it (written once, read once).  The two passes one by one come
from a kernel trace collected in a run of its own (the report quotes it); this file collects none.

    timeout -k 10 300 python tools/bench_tone_match.py [--rounds 3] [--out FILE]
"""
import argparse
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()

HBM_PEAK = 8.0e12
NAME = 'keep_tone_match_u8'
FACE_BYTES = 512 * 512 * 3


def kernel_alone(say, rounds=3, reps=20):
    from comfyui_keep_amd.engine import hiplib as L
    if NAME not in getattr(L, '_CV_SIGNATURES', {}):
        say(f"(this build has no {NAME}: the kernel part is skipped)")
        return
    from comfyui_keep_amd.engine.tone import tone_taps
    say(f"{NAME} alone: faces of 512 x 512 on noise, device events around one call (both passes), {rounds} rounds of the best of {reps}")
    say("launches after 3 warm ones.  floor = the bytes that must move at the 8 TB/s HBM peak: 3 x 786,432 per face without the int16")
    say("intermediate, 6 x with it (it is written once and read once; up to 32 faces it stays in the 256 MB Infinity Cache).")
    for sigma in (4, 16, 40):
        t = tone_taps(sigma)
        taps, R = (ctypes.c_int16 * len(t))(*t.tolist()), (len(t) - 1) // 2
        for F in (1, 3, 32):
            src = torch.randint(0, 256, (F, 512, 512, 3), dtype=torch.uint8, device='cuda')
            rst = torch.randint(0, 256, (F, 512, 512, 3), dtype=torch.uint8, device='cuda')
            out = torch.empty_like(rst)
            scratch = torch.empty((F, 512, 512, 3), dtype=torch.int16, device='cuda')
            for _ in range(3):
                L.call(NAME, src, rst, out, scratch, F, 512, 512, taps, R)
            torch.cuda.synchronize()
            per = []
            for _ in range(rounds):
                best = float('inf')
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    L.call(NAME, src, rst, out, scratch, F, 512, 512, taps, R)
                    e1.record()
                    e1.synchronize()
                    best = min(best, e0.elapsed_time(e1) * 1e-3)
                per.append(best / F)
            b = min(per)
            say(f"   sigma {sigma:2d} (R {R:3d})  {F:2d} faces  {[round(v * 1e6, 2) for v in per]} us per face, best {b * 1e6:7.2f}   "
                f"of the peak: {3 * FACE_BYTES / b / HBM_PEAK:5.3f} (3 x)  {6 * FACE_BYTES / b / HBM_PEAK:5.3f} (6 x)   "
                f"floor {3 * FACE_BYTES / HBM_PEAK * 1e6:.2f} / {6 * FACE_BYTES / HBM_PEAK * 1e6:.2f} us")
            del src, rst, out, scratch
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tone_match.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tone_match.py measures on the MI355X: no HIP device visible"
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def say(line=''):
        print(line, flush=True)
        lines.append(line)
    title = f"Tone match kernel (keep_tone_match_u8): restored faces keep the source crop's low band, {torch.cuda.get_device_name(0)}"
    say(title)
    say('=' * min(len(title), 140))
    say()
    say(f"Command: python tools/bench_tone_match.py --rounds {a.rounds}   ({time.strftime('%Y-%m-%d')})")
    say("No counters were collected.  NOT measured: the effect on real video with real weights, and whether sigma 16 is a good value.")
    say()
    kernel_alone(say, a.rounds)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
