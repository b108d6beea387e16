#!/usr/bin/env python
"""What the alias-free paste-back (KEEP_AMD_PASTE_AA: every shrunk face is area-sampled, N x N sub-samples per frame pixel) costs on
the MI355X, written as a text report (default profiles/paste_aa.txt).  No figure is fixed in advance: the numbers are reported.

1. The kernel alone -- one ``keep_paste_face_aa`` launch against one ``keep_paste_face`` launch on the same crop -> frame matrix (the
   single tap on it, the N x N sub-samples on its ``ss_affine``), a 1080p float frame, one rotated face at r = 0.7, 0.35 and 0.176
   (N = 2, 4, 8), between device events, the two entries alternating launch by launch, best of the launches per round.  In the same run:
   ``keep_u8_to_f32`` plus ``keep_f32_round_u8`` on that frame -- the two full-frame passes every paste makes around its blends.

2. ``GpuPaster.paste`` on the 1080p / 3-face paste case (engine/synth.py; r = 0.45, 0.30, 0.62), ``aa`` off and on, alternating, device
   events around the call.

3. ``process_frames_u8`` end to end (synthetic weights, tools/synth_facehelper.py) at 720p / 1 face / 96 frames (r = 0.49, N = 4), knob
   off and on, one processor each, warmed, interleaved round by round in one process, host clock around a synchronise.

    timeout -k 10 900 python tools/bench_paste_aa.py [--rounds 3] [--frames 96] [--kernel 1] [--paster 1] [--e2e 1] [--out FILE]
"""
import argparse
import ctypes as C
import math
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

CORE, NAME = 'keep_paste_face', 'keep_paste_face_aa'
SETTINGS = [('knob off', {}), ('paste aa', {'KEEP_AMD_PASTE_AA': '1'})]


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternating(a, b, rounds, reps, warm=5):
    """Best of ``reps`` per round for two timed thunks that alternate launch by launch, either one first in turn."""
    for _ in range(warm):
        a(), b()
    best = ([], [])
    for _ in range(rounds):
        t = ([], [])
        for r in range(reps):
            for k in ((0, 1) if r % 2 == 0 else (1, 0)):
                t[k].append((a, b)[k]())
        best[0].append(min(t[0]))
        best[1].append(min(t[1]))
    return best


def us(vs):
    return [round(v * 1e6, 2) for v in vs]


def kernel_alone(say, rounds=3, reps=30):
    from comfyui_keep_amd.engine import hiplib as L
    from comfyui_keep_amd.engine import paste, synth
    H, W = 1080, 1920
    frame, faces, _, classes = synth.synth_paste_case(H, W, 1)
    gp = paste.GpuPaster('cuda')
    face = torch.from_numpy(faces[0]).cuda()
    mask = gp.soft_masks(torch.from_numpy(classes).cuda())[0]
    frame_dev = torch.from_numpy(frame).cuda()
    acc0 = torch.from_numpy(frame.astype(np.float32)).cuda()
    acc = acc0.clone()
    out_u8 = torch.empty_like(frame_dev)
    one = C.c_float(1.0)

    def passes():
        L.call('keep_u8_to_f32', frame_dev, acc, frame_dev.numel())
        L.call('keep_f32_round_u8', acc, out_u8, acc.numel())
    say(f"one face per launch on a 1080p float frame, parse-mask form, opacity 1.0, rotated by 0.15 rad; device events, the entries alternate")
    say(f"launch by launch, either one first in turn, best of {reps} per round after 5 warm ones, {rounds} rounds (us per launch)")
    worst = 0.0
    for r in (0.7, 0.35, 0.176):
        a, b = r * math.cos(0.15), r * math.sin(0.15)
        M = np.array([[a, -b, W * 0.5 - (a - b) * 256 + 0.37], [b, a, H * 0.5 - (a + b) * 256 - 0.21]], np.float64)
        n = paste.aa_factor(M)
        box = paste.face_box(M, 512, 512, W, H)
        d2s = (C.c_double * 6)(*paste.invert_affine(M).reshape(-1).tolist())
        fine = (C.c_double * 6)(*paste.invert_affine(paste.ss_affine(M, n)).reshape(-1).tolist())

        def core():
            return events(lambda: L.call(CORE, acc, H, W, face, mask, 512, 512, d2s, *box, paste.PARSE_BORDER))

        def aa():
            return events(lambda: L.call(NAME, acc, H, W, face, mask, 512, 512, fine, *box, paste.PARSE_BORDER, n, one))
        acc.copy_(acc0)
        best = alternating(core, aa, rounds, reps)
        px = (box[2] - box[0]) * (box[3] - box[1])
        t = min(best[1])
        worst = max(worst, t)
        say(f"   r {r:5.3f} N {n}  box {box[2] - box[0]} x {box[3] - box[1]} = {px} px, {px * n * n} sub-samples")
        say(f"      {CORE:20s} {us(best[0])} best {min(best[0]) * 1e6:.2f}")
        say(f"      {NAME:20s} {us(best[1])} best {t * 1e6:.2f}   aa / core {t / min(best[0]):.2f}   "
            f"{t * 1e9 / (px * n * n):.3f} ns per sub-sample, {px * n * n * 16 / t * 1e-9:.0f} G tap loads/s")
    both = [events(passes) for _ in range(5)]
    both = [min(events(passes) for _ in range(reps)) for _ in range(rounds)]
    say(f"   keep_u8_to_f32 + keep_f32_round_u8 on the frame ({frame_dev.numel() * 10 / 1e6:.1f} MB moved): {us(both)} best {min(both) * 1e6:.2f}")
    if worst > min(both):
        say(f"   the dearest AA launch ({worst * 1e6:.2f} us) costs MORE than the two full-frame passes together ({min(both) * 1e6:.2f} us).  What bounds it,")
        say("   by the instruction mix (no counters were collected): every sub-sample is the whole coordinate arithmetic of a frame pixel -- 10")
        say("   float64 products / sums and 4 float64 -> int64 roundings -- plus 12 byte loads of the face and 4 guarded dword loads of the mask;")
        say("   the crop and its mask (1.8 MB) stay in L2, so the launch is bound by FP64 / integer VALU work and load issue, not by HBM.")
    else:
        say(f"   every AA launch costs less than the two full-frame passes together ({min(both) * 1e6:.2f} us), which every paste already makes.")
        say("   By the instruction mix (no counters were collected) a sub-sample is 10 float64 products / sums, 4 float64 -> int64 roundings, 12")
        say("   byte loads of the face and 4 guarded dword loads of the mask out of L2 (crop + mask: 1.8 MB): VALU and load issue, not HBM.")


def paster(say, rounds=3, reps=10):
    from comfyui_keep_amd.engine import paste, synth
    frame, faces, mats, classes = synth.synth_paste_case()
    gp = paste.GpuPaster('cuda')
    frame_dev, faces_dev, cls = torch.from_numpy(frame).cuda(), torch.from_numpy(faces).cuda(), torch.from_numpy(classes).cuda()
    mats = list(mats)
    best = alternating(lambda: events(lambda: gp.paste(frame_dev, faces_dev, mats, cls)),
                       lambda: events(lambda: gp.paste(frame_dev, faces_dev, mats, cls, aa=True)), rounds, reps, warm=3)
    say(f"GpuPaster.paste, 1080p / 3 faces (N = {[paste.aa_factor(M) for M in mats]}), frame, faces and class maps resident: device events around the call (mask blurs,")
    say(f"u8 -> f32, 3 blends, round), aa off and on alternating, best of {reps} per round, {rounds} rounds (us per call)")
    say(f"   aa off {us(best[0])} best {min(best[0]) * 1e6:.1f}")
    say(f"   aa on  {us(best[1])} best {min(best[1]) * 1e6:.1f}   on / off {min(best[1]) / min(best[0]):.3f}")


def end_to_end(rounds, n, say, flush):
    import synth_facehelper as SF
    from comfyui_keep_amd.engine import synth
    from comfyui_keep_amd.engine.arch import DEFAULT_ARCH
    from comfyui_keep_amd.engine.net import KeepNet
    dev = torch.device('cuda', torch.cuda.current_device())
    net = KeepNet(**DEFAULT_ARCH)
    net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
    net.to(dev).eval()
    H, W, faces = 720, 1280, 1
    procs = []
    for label, env in SETTINGS:                                     # the knob is read in the constructor: one processor per setting
        os.environ.pop('KEEP_AMD_PASTE_AA', None)
        os.environ.update(env)
        proc, helper = SF.make_processor(net, (H, W), faces)
        helper.resize_for_detector = None                           # the processor resizes the detector inputs, as with the reference helper
        proc.gpu_resize = proc.gpu_detect_resize = True
        procs.append((label, proc, helper))
    os.environ.pop('KEEP_AMD_PASTE_AA', None)
    frames = [f for f in np.random.default_rng(0).integers(0, 256, (n, H, W, 3), dtype=np.uint8)]

    def run(proc, helper):
        helper.begin_sequence()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = proc.process_frames_u8(frames, 1.0, False, False, False, max_clip_length=20)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert isinstance(res, torch.Tensor) and res.shape[0] == n and proc.frame_store is True
        return dt
    say(f"720p, 1 face, {n} frames, factor 1.0, max_clip_length 20 (seconds per call)")
    for _, proc, helper in procs:
        run(proc, helper)
    t = {label: [] for label, _, _ in procs}
    for _ in range(rounds):
        for label, proc, helper in procs:
            t[label].append(run(proc, helper))
    for label, proc, _ in procs:
        rs = t[label]
        say(f"   {label:9s} {[round(v, 4) for v in rs]} best {min(rs):.4f} ({n / min(rs):6.1f} frames/s)  spread {max(rs) - min(rs):.4f}   "
            f"last_paste_aa {getattr(proc, 'last_paste_aa', None)}")
    say(f"   on / off: {min(t['paste aa']) / min(t['knob off']):.3f}")
    flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--kernel', type=int, default=1)
    ap.add_argument('--paster', type=int, default=1)
    ap.add_argument('--e2e', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'paste_aa.txt'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_paste_aa.py measures on the MI355X: no HIP device visible"
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def flush():
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    def say(line=''):
        print(line, flush=True)
        lines.append(line)
    title = f"Alias-free paste-back (KEEP_AMD_PASTE_AA): shrunk faces are area-sampled, {torch.cuda.get_device_name(0)}"
    say(title)
    say('=' * min(len(title), 140))
    say()
    say(f"Command: python tools/bench_paste_aa.py --rounds {a.rounds} --frames {a.frames} --kernel {a.kernel} --paster {a.paster} "
        f"--e2e {a.e2e}   ({time.strftime('%Y-%m-%d')})")
    say("No counters were collected.  Not measurable here: the visual effect on real video with real weights (less shimmer on the restored")
    say("face is the aim; the synthetic checkerboard of tests/test_paste_aa_host.py is what is proved).")
    say()
    say("Compiled for gfx950 (-Rpass-analysis=kernel-resource-usage), paste_aa_kernel<N>, 256 threads, no LDS, no scratch:")
    say("   N = 2:  25 VGPRs, 58 SGPRs, occupancy 8 waves / SIMD      (4 lanes per frame pixel, 1 sub-sample per lane)")
    say("   N = 4:  25 VGPRs, 58 SGPRs, occupancy 8 waves / SIMD      (16 lanes per frame pixel, 1 sub-sample per lane)")
    say("   N = 8:  68 VGPRs, 54 SGPRs, occupancy 7 waves / SIMD      (16 lanes per frame pixel, 4 sub-samples per lane)")
    say()
    if a.kernel:
        kernel_alone(say, a.rounds)
        say()
        flush()
    if a.paster:
        paster(say, a.rounds)
        say()
        flush()
    if a.e2e:
        say("End to end process_frames_u8: host clock around a synchronise, synthetic weights, both settings warmed, then they alternate round")
        say("by round in one process.")
        end_to_end(a.rounds, a.frames, say, flush)
    flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
