#!/usr/bin/env python
"""bench.py -- headline metric of BASELINE.json: restored 512x512 face frames/s on T=20 clips.

    python bench.py --gpus 1 --steps K --warmup W [--clips B] [--precision x3|fp32|bf16] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

A plain run sets up, warms up, times K steps, writes the last step's output if --dump-outputs is given and prints the JSON
line: the headline keys, `ms_per_step` (wall milliseconds of one timed step) and what falls out of the timing for free.
Everything that takes runs of its own -- roofline, the other policies, the legs listed below, cpu_baseline and, under
--gpus N, the one-video-per-GPU leg -- runs only with --full (--no-extras / --no-cpu-baseline trim --full).

--dump-outputs DIR: DIR/restored_frames.npy (float32) holds the restored frames the last timed step returned -- whole when they
fit in DUMP_BYTES, else a fixed sample of them (dump_outputs); the inputs are a pure function of the arguments, so two builds
run with the same arguments can be compared output for output.

One "step" = one pass of the hot path (KEEP.forward on the HIP engine) over one batch of synthetic input:
B independent 20-frame 512x512 clips per GPU (config.workload, BASELINE configs[1]), inputs already resident in HBM.
Multi-GPU is weak scaling: every rank restores its OWN B clips (distinct seeds; BASELINE configs[4] at B = 15); the only
collective is the one-off RCCL broadcast of the packed weights, outside the timed region and reported as
`broadcast_ms`.  value = (N * B * 20 * K) / max-over-ranks wall time.

Precision policy of `value` (default `x3`): every matrix-core operand split into two fp16 halves, three MFMAs per
product, fp32 accumulate -- fp32-grade products on the 16-bit matrix pipe.  It passes the SAME <= 1e-3 parity tests as the
exact-f32 policy (tests/test_gpu_net.py runs every network test on both); `dtype` says "f16x3".  With --full the exact-f32
policy and the bf16 speed policy (outside the parity tolerance) are timed in the same invocation and reported beside it,
each with its live agreement with the exact-f32 result on the same input.

Also on the JSON line with --full:
  roofline       dominant kernel (conv3x3_halo_x3s_kernel, the streaming LDS-halo 3x3 convolution on split fp16): algorithmic FLOPs of
                 its launches in one step / their summed HIP-event durations (events on the launch stream), against the
                 dense fp16 MFMA peak divided by the three MFMAs every product costs (2500 / 3 TFLOP/s); `mfma_frac` is
                 the same quotient in raw matrix-pipe terms (3 x achieved / 2500);
  b1             the literal configs[1] case: ONE 20-frame clip in flight;
  configs        BASELINE configs[2] / [3] as hot-path workloads through the processor's own chunking: 300 crops
                 (15 clips) and 900 frame-major interleaved crops of 3 faces (45 clips), uint8 host -> uint8 host;
  facelib        ParseNet / RetinaFace on the engine, batched
  cpu_baseline   the CPU oracle (a port of the reference algorithm, PyTorch-CPU fp32) on the benchmarked clip
                 (one T=20 clip, ~1 min), rank 0 / N=1 only -- a reported baseline, not the target.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from comfyui_keep_amd.engine import dist as kdist  # noqa: E402
from comfyui_keep_amd.engine import synth  # noqa: E402
from comfyui_keep_amd.engine.arch import DEFAULT_ARCH  # noqa: E402
from comfyui_keep_amd.engine.net import KeepNet  # noqa: E402

T_CLIP = 20
PEAK_16BIT_MFMA_TFLOPS = 2500.0       # dense bf16 / fp16 MFMA (no sparsity), MI355X_MICROARCH.md
PEAK_F32_MFMA_TFLOPS = 157.3          # v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD
FLOP_PER_FRAME_T20 = 1038.5e9         # SURVEY.md 8d (reference graph, 2 FLOP/MAC)
GMFLOW_DUPLICATE_FLOP_PER_FRAME = 33.0e9   # backbone passes of interior frames the reference repeats: 18 of 38 per T=20 clip
PEAK = {'fp32': PEAK_F32_MFMA_TFLOPS, 'bf16': PEAK_16BIT_MFMA_TFLOPS, 'x3': PEAK_16BIT_MFMA_TFLOPS / 3.0}
DTYPE = {'fp32': 'f32', 'bf16': 'bf16', 'x3': 'f16x3'}
PMC_FILE = os.path.join(ROOT, 'profiles', 'r06_pmc_traffic.json')
DUMP_BYTES = 48 << 20                 # --dump-outputs: bytes written in all, over every rank


def _s64(v):
    """A uint64 value as the int64 with the same bits."""
    v = int(v)
    return v - (1 << 64) if v >= 1 << 63 else v


def _lsr64(z, k):
    """Logical right shift of int64 tensors that hold uint64 bit patterns."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _splitmix64_t(z):
    """synth._splitmix64 on int64 tensors (two's-complement wrap-around = the uint64 arithmetic of the original)."""
    z = z + _s64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr64(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr64(z, 27)) * _s64(0x94D049BB133111EB)
    return z ^ _lsr64(z, 31)


def synth_clip_device(T, B, seed, phase, device):
    """synth.synth_clip(T, B, seed=seed, phase=phase) -- the 512 x 512 texture clips -- bit for bit, computed on `device`.  The
    NumPy original spends ~2.4 s of one host core per clip, two minutes for the 48 clips of a step.  Here the sampling grid of a
    frame (the same for every clip: it depends on t and phase only) is computed on the host by the original's float64 operations,
    on one row and one column; the lattice gathers, interpolation, hash noise and clipping run on the device for all clips at
    once, one torch op per NumPy op, in the original's order (no fused forms).  tests/test_bench.py pins it to synth_clip."""
    S = 512
    cells, amps = (9, 17, 33), (0.5, 0.6, 0.5)
    grid = np.arange(S, dtype=np.float64)
    tabs = [torch.from_numpy(np.stack([np.stack([synth.uniform_pm1(f'tex:{b}:{oi}:{ch}', (S // c + 8) ** 2, seed).reshape(S // c + 8, S // c + 8)
                                                 for ch in range(3)]) for b in range(B)])).to(device) for oi, c in enumerate(cells)]
    idx = torch.arange(S * S, dtype=torch.int64, device=device)
    out = torch.empty((B, T, 3, S, S), dtype=torch.float32, device=device)
    for t in range(T):
        X = grid - (synth.CLIP_MOTION[0] * t + phase)
        Y = grid - (synth.CLIP_MOTION[1] * t + 0.7 * phase)
        img = torch.zeros((B, 3, S, S), dtype=torch.float64, device=device)
        for oi, c in enumerate(cells):
            gx, gy = X / c + 3.0, Y / c + 3.0
            ix, iy = np.floor(gx), np.floor(gy)
            fx, fy = gx - ix, gy - iy
            fx, fy = fx * fx * (3.0 - 2.0 * fx), fy * fy * (3.0 - 2.0 * fy)
            ix = torch.from_numpy(ix.astype(np.int64)).to(device)[None, :]
            iy = torch.from_numpy(iy.astype(np.int64)).to(device)[:, None]
            fx = torch.from_numpy(fx).to(device)
            fy = torch.from_numpy(fy).to(device)[:, None]
            tb = tabs[oi]
            top = tb[:, :, iy, ix] * (1.0 - fx) + tb[:, :, iy, ix + 1] * fx
            bot = tb[:, :, iy + 1, ix] * (1.0 - fx) + tb[:, :, iy + 1, ix + 1] * fx
            img += amps[oi] * (top * (1.0 - fy) + bot * fy)
        keys = torch.tensor([[_s64(synth._name_key(f'clip:{b}:{t}:{ch}', seed)) for ch in range(3)] for b in range(B)],
                            dtype=torch.int64, device=device)[:, :, None]
        bits = _splitmix64_t(_splitmix64_t(idx ^ keys) + keys)
        u = (_lsr64(bits, 40).to(torch.float64) + 0.5) * (2.0 / 16777216.0) - 1.0          # synth.uniform_pm1
        out[:, t] = (img + 0.002 * u.view(B, 3, S, S)).clamp_(-1.0, 1.0).to(torch.float32)
    return out


def dump_outputs(out, path, rank, world):
    """--dump-outputs: the restored frames the last timed step returned ([B, T, 3, 512, 512] float32, 3 GB at 48 clips) as
    PATH/restored_frames.npy (restored_frames_rank<r>.npy per rank under --gpus N): the whole array when it fits in this rank's
    share of DUMP_BYTES, else a fixed sample, flat and in order -- one element from each of equal runs of the flattened array, at
    an offset drawn by a generator seeded with 0, so every run with the same --clips samples the same positions."""
    flat = out.reshape(-1)
    n = DUMP_BYTES // world // flat.element_size()
    if flat.numel() > n:
        run = -(-flat.numel() // n)
        k = flat.numel() // run
        pos = torch.arange(k, dtype=torch.int64) * run + torch.randint(0, run, (k,), generator=torch.Generator().manual_seed(0))
        out = flat[pos.to(flat.device)]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, 'restored_frames.npy' if world == 1 else f'restored_frames_rank{rank}.npy'), out.cpu().numpy())


FAKE = os.environ.get('KEEP_BENCH_FAKE_NET') == '1'     # tests/test_dist_gloo.py: the N-rank plumbing of this file on a machine without a GPU


class _FakeBenchNet:
    """KEEP_BENCH_FAKE_NET=1: stands in for KeepNet so that `bench.py --gpus N` can be driven over gloo on CPU -- rendezvous, the chunked
    weight broadcast and its checksum, max-over-ranks timing, the per-rank gather, the one-video-per-GPU leg and the line's keys are the
    real code; only the forward is a stand-in (and the line says so: "fake_engine": true, no roofline)."""
    precision, x3_fallbacks, shard_across_ranks = 'x3', 0, True

    def __init__(self):
        self._index, self._blob = None, None

    def load(self):
        n = int(float(os.environ.get('KEEP_BENCH_FAKE_BLOB_MB', '3.5')) * (1 << 20)) // 4
        self._index, self._blob = {'fake.weight': (0, (n,))}, torch.arange(n, dtype=torch.float32)

    def packed_blob(self):
        return self._blob

    def adopt_packed(self, index, blob):
        self._index, self._blob = index, blob

    def set_precision(self, p):
        self.precision = p
        return self

    def eval(self):
        return self

    def __call__(self, x):
        time.sleep(0.002 * x.shape[0])
        return 1.0 - x

    def run_clips_u8(self, clips, max_b=None):
        time.sleep(0.002 * len(clips))
        return [255 - c for c in clips]


def _sync():
    if not FAKE:
        torch.cuda.synchronize()


def build_net(rank, world):
    net = _FakeBenchNet() if FAKE else KeepNet(**DEFAULT_ARCH)
    bcast = None
    if rank == 0:
        if FAKE:
            net.load()
        else:
            net.load_state_dict(synth.synth_state_dict(seed=0), strict=True)
            net.to(torch.device('cuda', torch.cuda.current_device()))
        index, blob = net._index, net.packed_blob()
    else:
        index, blob = None, None
    if world > 1:
        _sync()
        torch.distributed.barrier()
        t0 = time.perf_counter()
        index, blob = kdist.broadcast_packed_weights(index, blob, src=0)
        _sync()
        torch.distributed.barrier()
        bcast = {"ms": (time.perf_counter() - t0) * 1e3}
        if rank != 0:
            net.adopt_packed(index, blob)
        # the first real ncclBroadcast between GPUs is the driver's 8-GPU run: every rank reports an exact checksum of what it holds
        # (int32 view, int64 sum) and rank 0 compares them -- a broadcast that moved wrong bytes shows up in the line, not in the pixels
        flat = net.packed_blob().view(-1)
        mine = flat.view(torch.int32).sum(dtype=torch.int64).reshape(1).to('cuda' if torch.distributed.get_backend() == 'nccl' else 'cpu')
        sums = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(sums, mine)
        bcast.update(kdist.LAST_BROADCAST)
        bcast["verified"] = bool(all(int(t.item()) == int(sums[0].item()) for t in sums))
        bcast["mb"] = flat.numel() * 4 / 1e6
    return net.eval(), bcast


def conv_roofline(net, x):
    """One instrumented step: every keep_conv2d launch bracketed by HIP events on the launch stream, grouped by the kernel
    family keep_conv2d_plan names (what rocprofv3 prints).  The dominant kernel is the one with the largest summed
    duration; `achieved` = its algorithmic FLOPs / its summed event durations."""
    net.o.profile = []
    net(x)
    torch.cuda.synchronize()
    rec, net.o.profile = net.o.profile, None
    by = {}
    for cfg, flops, split_k, e0, e1, nbytes, *_ in rec:
        d = by.setdefault(cfg, [0.0, 0.0, 0, 0.0])
        d[0] += flops
        d[1] += e0.elapsed_time(e1) * 1e-3          # split-K launches include their reduce kernel
        d[2] += 1
        d[3] += nbytes
    key = max(by, key=lambda k: by[k][1])
    peak = PEAK[net.precision]
    flops, secs, n, nbytes = by[key]
    tf = flops / secs / 1e12
    # HBM bytes per launch of this kernel: rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE, separate runs of
    # tools/run_step.py on the same step; profiles/refresh.sh) -- a PMC session cannot run inside this process.  Reported
    # only for an exact (policy, clips per GPU, kernel family) match, else null with the reason.
    traffic, traffic_note = None, f'no PMC record for policy {net.precision}'
    try:
        pmc = json.load(open(PMC_FILE))[net.precision]
        fam = [v for k, v in pmc['kernels'].items() if k == key or k.startswith(key.rstrip('>') + ',') or k.startswith(key + '<')]
        if pmc['clips_per_gpu'] != x.shape[0]:
            traffic_note = f"PMC passes were taken at {pmc['clips_per_gpu']} clips per GPU, this run uses {x.shape[0]}"
        elif not fam:
            traffic_note = f'kernel {key} not in {os.path.basename(PMC_FILE)} (kernel renamed since the PMC passes?)'
        else:
            n_l = sum(v['launches'] for v in fam)
            traffic = round(sum(v['hbm_bytes_per_launch'] * v['launches'] for v in fam) / n_l)
            traffic_note = f'PMC: 2*FETCH_SIZE + WRITE_SIZE per launch, {os.path.basename(PMC_FILE)}'
    except (OSError, KeyError, ValueError):
        pass
    tot_f = sum(v[0] for v in by.values())
    tot_s = sum(v[1] for v in by.values())
    detail = {k: {"launches": v[2], "gflop": round(v[0] / 1e9, 1), "ms": round(v[1] * 1e3, 2),
                  "tflops": round(v[0] / v[1] / 1e12, 1), "algorithmic_gb_per_s": round(v[3] / v[1] / 1e9, 1)}
              for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])}
    # nearest x2 + 3x3 as four 2x2-tap phase convolutions (x3 policy, keep_hip.h KEEP_UPSAMPLE_X2_PHASES): `gflop` / `tflops` price the
    # reference's 9 taps (algorithmic), 4 of 9 are multiplied
    skipped = 0.0
    for k, v in by.items():
        if 'x2 phases' in k:
            detail[k]["executed_gflop"] = round(v[0] * 4.0 / 9.0 / 1e9, 1)
            detail[k]["executed_tflops"] = round(v[0] * 4.0 / 9.0 / v[1] / 1e12, 1)
            skipped += v[0] * 5.0 / 9.0
    out = {"bound": "mfma", "kernel": key,
           "achieved": round(tf, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(tf / peak, 4),
           "traffic": traffic, "traffic_note": traffic_note,
           "algorithmic_bytes_per_launch": round(nbytes / n), "launches_per_step": n,
           "avg_launch_ms": round(secs / n * 1e3, 4), "algorithmic_gflop_per_launch": round(flops / n / 1e9, 2),
           "conv_path_tflops": round(tot_f / tot_s / 1e12, 2), "conv_path_frac": round(tot_f / tot_s / 1e12 / peak, 4),
           "conv_path_ms": round(tot_s * 1e3, 1), "conv_path_tflops_executed": round((tot_f - skipped) / tot_s / 1e12, 2),
           "skipped_gflop_per_step": round(skipped / 1e9, 1), "all_conv_kernels": detail}
    if net.precision == 'x3':
        out["peak_note"] = ("dense fp16 MFMA peak 2500 TFLOP/s / 3: every fp32-grade product costs three fp16 MFMAs "
                            "(hi*hi + hi*lo + lo*hi); `achieved` counts algorithmic FLOPs once")
        out["mfma_frac"] = round(3.0 * tf / PEAK_16BIT_MFMA_TFLOPS, 4)
        out.update(practical_peak_x3(tf))
    return out


_PRACTICAL = {}


def practical_peak_x3(achieved_tf):
    """BESIDE the nominal peak (never instead of it): what the x3 product loop of the dominant kernel sustains on THIS box, in this
    process, when everything but its MFMAs and LDS fragment reads is removed (tools/dev/x3_ceiling_probe.hip, variant 1, two blocks per CU,
    random operands; built by __graft_entry__.build()).  profiles/r06_x3_ceiling_probe.txt holds the full table."""
    if not _PRACTICAL:
        try:
            import importlib.util
            spec = importlib.util.spec_from_file_location('x3_ceiling', os.path.join(ROOT, 'tools', 'dev', 'x3_ceiling.py'))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            loop, bare = mod.practical_peak()
            torch.cuda.synchronize()
            _PRACTICAL.update(ok=True, loop=loop, bare=bare)
        except Exception as e:      # no probe library on this box: say so, do not guess
            _PRACTICAL.update(ok=False, why=f'{type(e).__name__}: {e}')
    if not _PRACTICAL['ok']:
        return {"practical_peak": None, "frac_of_practical": None, "practical_peak_note": "x3 ceiling probe unavailable (" + _PRACTICAL['why'] + ")"}
    loop, bare = _PRACTICAL['loop'], _PRACTICAL['bare']
    return {"practical_peak": round(loop['x3_tflops'], 1), "frac_of_practical": round(achieved_tf / loop['x3_tflops'], 4),
            "practical_peak_note": ("measured in this run: the halo kernels' x3 product loop with its operands resident in LDS and nothing else (12 MFMAs + 8 "
                                    "ds_read_b128 per tap and wave, random data, two blocks per CU) sustains %.0f TFLOP/s of raw MFMA rate at an in-kernel %.2f GHz = "
                                    "%.0f x3-equivalent; a bare MFMA loop on random register operands %.0f raw at %.2f GHz.  `peak` / `frac` stay the nominal 2500 / 3"
                                    % (loop['raw_tflops'], loop['clock_ghz'], loop['x3_tflops'], bare['raw_tflops'], bare['clock_ghz'])),
            "bare_mfma_loop_tflops": round(bare['raw_tflops'], 1), "bare_mfma_loop_clock_ghz": round(bare['clock_ghz'], 3),
            "x3_loop_clock_ghz": round(loop['clock_ghz'], 3)}


def cpu_baseline(Tc):
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import keep_oracle as O
    W = synth.synth_state_dict(seed=0)
    x = synth.synth_clip(T=Tc, B=1, seed=1234)
    threads = max(1, min(int(os.environ.get('KEEP_BENCH_CPU_THREADS', '32')), os.cpu_count() or 1))
    torch.set_num_threads(threads)      # beyond ~32 threads the CPU convolutions are memory-bound and slow down
    t0 = time.time()
    O.keep_forward(x, W)
    dt = time.time() - t0
    return {"value": round(Tc / dt, 4), "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": f"one B=1 T={Tc} 512x512 synthetic clip ({Tc} frames, {dt:.1f}s, torch CPU fp32, {threads} threads of "
                      f"{os.cpu_count()} logical cores); {(648.8 + (Tc - 1) * 1059.0) / Tc:.0f} GFLOP/frame"}


def synth_crops(n, seed=0):
    """n uint8 BGR 512x512 crops (smooth moving pattern + noise, like synth_clip) for the processor-level legs."""
    g = torch.Generator().manual_seed(seed)
    base = torch.from_numpy(synth.ramp_image()).to(torch.int16)
    out = []
    for k in range(n):
        noise = torch.randint(-20, 21, (512, 512, 3), generator=g, dtype=torch.int16)
        out.append(((torch.roll(base, shifts=(3 * k) % 512, dims=1) + noise) % 256).to(torch.uint8).numpy())
    return out


def paste_leg(frames=10):
    """SURVEY 8f-2 / BASELINE configs[3] post-processing: one 1080p frame with 3 restored faces composited on the GPU
    (engine/paste.py: parse-mask blurs, inverse-affine warps, blend), host uint8 in -> host uint8 out per frame."""
    from comfyui_keep_amd.engine.paste import GpuPaster
    frame, faces, mats, classes = synth.synth_paste_case()
    gp = GpuPaster('cuda')
    cls = torch.from_numpy(classes).cuda()                 # ParseNet's arg-max lives on the device in the product path
    gp.paste(frame, faces, list(mats), cls)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        out = gp.paste(frame, faces, list(mats), cls).cpu()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / frames
    return {"ms_per_frame": round(dt * 1e3, 3), "frames_per_s": round(1.0 / dt, 1), "frame": "1920x1080, 3 faces",
            "what": "host uint8 frame + 3 restored uint8 crops -> composited host uint8 frame (H2D, 6 Gaussian passes of 101 taps, "
                    "3 box warps + blends, D2H); arithmetic bit-equal to oracle/paste_oracle.py, unpinned against cv2 (absent)"}


def facelib_leg():
    """the face-analysis networks either side of the hot path on the engine, batched (synthetic weights):
    ParseNet(512, 512) class maps for 16 faces per call, RetinaFace(resnet50) raw outputs + host decode / NMS for 16 video
    frames per call at 640 x 1138 (a 720p frame after the helper's resize-to-640 rule, face_restoration_helper.py:206-213)."""
    from comfyui_keep_amd.engine import parsenet as PN
    from comfyui_keep_amd.engine import retinaface as RF
    out = {}
    eng = PN.ParseNetEngine(PN.synth_parsenet_state_dict(seed=0)).to('cuda')
    x = torch.rand((16, 512, 512, 3), device='cuda') * 2 - 1
    eng.classes(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        eng.classes(x)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    out["parsenet_512"] = {"faces_per_s": round(16 / dt, 1), "ms_per_call": round(dt * 1e3, 2), "batch": 16,
                           "what": "fp32 NHWC faces on the device -> uint8 class maps on the device (x3 policy)"}
    del eng, x
    det = RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0)).to('cuda')
    frames = torch.randint(0, 256, (16, 640, 1138, 3), dtype=torch.uint8)
    det.detect_batch(frames, 0.97)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        det.detect_batch(frames, 0.97)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    x = torch.rand((16, 640, 1138, 3), device='cuda') * 255 - 110
    det.raw_heads(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        det.raw_heads(x)
    torch.cuda.synchronize()
    dn = (time.perf_counter() - t0) / 3
    out["retinaface_resnet50_640x1138"] = {"frames_per_s": round(16 / dt, 1), "ms_per_call": round(dt * 1e3, 2), "batch": 16,
                                           "network_only_frames_per_s": round(16 / dn, 1),
                                           "what": "uint8 BGR frames in host memory -> boxes + 5 landmarks per frame on the host "
                                                   "(pinned staging + H2D, network, scores / threshold / prior decode, score ordering "
                                                   "and NMS on the device, D2H of the kept detections: ~110 per frame with the synthetic "
                                                   "weights -- a real video has a handful); network_only: device tensor in, head "
                                                   "rows on the device out"}
    del det
    # retinaface_mobile0.25 (detection/__init__.py:38-41): the same pipeline on the MobileNetV1 x0.25 trunk
    det = RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0, backbone='mobile0.25')).to('cuda')
    det.detect_batch(frames, 0.97)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        det.detect_batch(frames, 0.97)
    torch.cuda.synchronize()
    dmh = (time.perf_counter() - t0) / 3
    det.raw_heads(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        det.raw_heads(x)
    torch.cuda.synchronize()
    dm = (time.perf_counter() - t0) / 5
    out["retinaface_mobile0.25_640x1138"] = {"frames_per_s": round(16 / dmh, 1), "network_only_frames_per_s": round(16 / dm, 1),
                                             "ms_per_call": round(dmh * 1e3, 2), "batch": 16,
                                             "what": "as above (uint8 frames in host memory -> detections on the host); network_only: "
                                                     "depthwise 3x3 kernel + 1x1 GEMMs + LeakyReLU(0.1) epilogues"}
    del det, x
    # YOLOv5n / YOLOv5l face detectors (detection/__init__.py:42-49): YoloDetector.detect_faces on a 720p frame after the helper's resize
    # (640 x 1137 uint8 in host memory -> letterboxed to 704 x 1152 on the device, face_detector.py:50-62 -> network -> selection + NMS on
    # the device -> kept rows on the host: engine/yoloface.py:yolo_detect_batch_device); network_only: device tensor in, decoded
    # [N, anchors, 16] predictions on the device out
    import types
    from comfyui_keep_amd.engine import yoloface as YF
    xy = torch.rand((16, 704, 1152, 3), device='cuda')
    yframes = torch.randint(0, 256, (16, 640, 1137, 3), dtype=torch.uint8)
    for name in ('YOLOv5n', 'YOLOv5l'):
        yolo = YF.YoloFaceEngine(YF.synth_yolo_state_dict(name, seed=0)).to('cuda')
        yolo.forward_nhwc(xy)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            yolo.forward_nhwc(xy)
        torch.cuda.synchronize()
        dy = (time.perf_counter() - t0) / 3
        ydet = types.SimpleNamespace(detector=YF.EngineYoloModel(yolo), target_size=None, min_face=10, device='cuda')
        for _ in range(2):
            YF.yolo_detect_batch(ydet, yframes, 0.97)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            YF.yolo_detect_batch(ydet, yframes, 0.97)
        torch.cuda.synchronize()
        dyh = (time.perf_counter() - t0) / 5
        out[f"{name.lower()}_face_640x1137"] = {"frames_per_s": round(16 / dyh, 1), "network_only_frames_per_s": round(16 / dy, 1),
                                                "ms_per_call": round(dyh * 1e3, 2), "batch": 16,
                                                "what": "uint8 frames in host memory -> detections on the host (letterbox kernel, network, "
                                                        "selection + NMS on the device; 0.97 threshold of the helper)"}
        del yolo, ydet
    return out


def pipeline_leg(net, n_frames, H, W, faces, batch=20):
    """BASELINE configs[2] / [3] END TO END on the engine, video frames in host memory -> restored video frames in host memory:
    RetinaFace(resnet50) on the frames resized to the helper's 640-px short side (engine/retinaface.py, device-side decode),
    the crop warp of every face (``keep_warp_affine_u8``), the clip loop (``run_clips_u8``: chunks of 20 crops per face track),
    ParseNet on the restored faces (engine/parsenet.py), the parse-mask paste-back (engine/paste.py), D2H of the frames.
    Synthetic frames, weights and face geometry (fixed crop <-> frame similarities per track: the detector's boxes on random
    weights are not faces; cv2's estimateAffinePartial2D / the landmark smoothing stay on the host in the product and are not
    on this leg); the frame resize in front of the detector is an area interpolation on the device (the helper's INTER_AREA)."""
    from comfyui_keep_amd.engine import parsenet as PN
    from comfyui_keep_amd.engine import retinaface as RF
    from comfyui_keep_amd.engine import hiplib as L
    from comfyui_keep_amd.engine.paste import GpuPaster, crop_faces, invert_affine
    dev = net.device
    det = RF.RetinaFaceEngine(RF.synth_retinaface_state_dict(seed=0)).to(dev)
    par = PN.ParseNetEngine(PN.synth_parsenet_state_dict(seed=0)).to(dev)
    paster = GpuPaster(dev)
    g = torch.Generator().manual_seed(faces)
    frames = torch.randint(0, 256, (n_frames, H, W, 3), generator=g, dtype=torch.uint8)
    sc = 640.0 / min(H, W)
    dh, dw = int(H * sc), int(W * sc)
    # crop -> frame similarities of the face tracks (face i: centre drifts slowly), scale so that a face spans ~0.35 of the height
    s0 = 0.35 * H / 512.0
    inv = [[np.array([[s0, 0.0, (0.25 + 0.25 * i) * W - 256 * s0 + 0.5 * t], [0.0, s0, 0.5 * H - 256 * s0 + 0.2 * t]], np.float64)
            for i in range(faces)] for t in range(n_frames)]

    def run():
        timings = {}
        t0 = time.perf_counter()
        n_det = 0
        for s in range(0, n_frames, 32):                      # 1. detection on the resized frames
            chunk = frames[s:s + 32].to(dev, non_blocking=True)
            small = torch.nn.functional.interpolate(chunk.permute(0, 3, 1, 2).float(), size=(dh, dw), mode='area')
            small = small.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
            n_det += sum(len(d) for d in det.detect_batch(small, 0.97))
        torch.cuda.synchronize()
        timings['detect_s'] = time.perf_counter() - t0
        t1 = time.perf_counter()
        crops = [[] for _ in range(faces)]                    # 2. crop warps, per face track
        for t in range(n_frames):
            c = crop_faces(frames[t], [invert_affine(m) for m in inv[t]], (512, 512), dev)
            for i in range(faces):
                crops[i].append(c[i])
        torch.cuda.synchronize()
        timings['crop_s'] = time.perf_counter() - t1
        t2 = time.perf_counter()
        clips = [torch.stack(tr[s:s + 20]) for tr in crops for s in range(0, n_frames, 20)]      # 3. the clip loop
        restored = net.run_clips_u8(clips)
        per_track = n_frames // 20 + (1 if n_frames % 20 else 0)
        tracks = [torch.cat(restored[i * per_track:(i + 1) * per_track]) for i in range(faces)]
        timings['restore_s'] = time.perf_counter() - t2
        t3 = time.perf_counter()
        out = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, pin_memory=True)
        for s in range(0, n_frames, batch):                   # 4. ParseNet + paste-back, D2H of the finished frames
            e = min(s + batch, n_frames)
            fb = torch.stack([tracks[i][t] for t in range(s, e) for i in range(faces)]).to(dev, non_blocking=True)
            x = torch.empty(fb.shape, dtype=torch.float32, device=dev)
            L.call('keep_img2tensor', fb, x, fb.numel() // 3)
            cls = par.classes(x)
            for k, t in enumerate(range(s, e)):
                o = paster.paste(frames[t], fb[k * faces:(k + 1) * faces], inv[t], cls[k * faces:(k + 1) * faces])
                out[t].copy_(o, non_blocking=True)
        torch.cuda.synchronize()
        timings['parse_paste_s'] = time.perf_counter() - t3
        timings['total_s'] = time.perf_counter() - t0
        return timings, n_det, out

    run()                                                     # warm: allocator, plan caches, pinned buffers
    tm, n_det, out = run()
    assert out.shape == (n_frames, H, W, 3)
    return {"value": round(n_frames / tm['total_s'], 2), "unit": "video frames/s", "frames": n_frames, "frame_size": [H, W],
            "faces_per_frame": faces, "restored_faces_per_s": round(n_frames * faces / tm['total_s'], 2),
            "seconds": {k: round(v, 3) for k, v in tm.items()},
            "what": "uint8 frames in host memory -> detect (RetinaFace on the engine) -> crop warp -> KEEP clip loop -> ParseNet -> "
                    "paste-back -> uint8 frames in host memory, every stage on the MI355X; synthetic face geometry"}


def product_leg(net, n_frames, H, W, faces):
    """BASELINE configs[2] / [3] through the PRODUCT's own sequence entry point: ``KEEPFaceProcessor.process_image_sequence`` (the
    node's call: float IMAGE tensor in host memory -> float IMAGE tensor in host memory) and ``process_frames_u8`` (the same between
    the two ComfyUI converters: uint8 frames -> uint8 frames, comparable with ``pipeline_leg``).  The reference's
    FaceRestoreHelper needs cv2 and the reference tree, neither of which exists on the GPU box: ``tools/synth_facehelper.py`` stands in
    for it -- same calls from the processor, the engine's RetinaFace / ParseNet behind it, synthetic landmarks (a detector with
    random weights finds no faces), Umeyama instead of cv2.estimateAffinePartial2D.  Everything else is the shipped code path:
    batched detection pre-pass, tracking + smoothing (modules/face_tracks.py), device crop warp, the streamed clip loop + ParseNet +
    paste-back (``_restore_and_paste_streamed``)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import synth_facehelper as SF
    proc, helper = SF.make_processor(net, (H, W), faces)
    g = torch.Generator().manual_seed(faces)
    frames_u8 = torch.randint(0, 256, (n_frames, H, W, 3), generator=g, dtype=torch.uint8)
    frames_list = [frames_u8[i].numpy() for i in range(n_frames)]

    def run_u8():
        helper.begin_sequence()
        t0 = time.perf_counter()
        out = proc.process_frames_u8(frames_list, 1.0, False, faces == 1, False, max_clip_length=20)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    run_u8()                                                  # warm: allocator, plan caches, pinned buffers
    d8, out8 = run_u8()
    assert tuple(out8.shape) == (n_frames, H, W, 3) and out8.dtype == torch.uint8
    assert int((out8 != frames_u8).any(-1).sum()) > n_frames * 1000          # faces were pasted
    rec = {"value": round(n_frames / d8, 2), "unit": "video frames/s", "frames": n_frames, "frame_size": [H, W], "faces_per_frame": faces,
           "restored_faces_per_s": round(n_frames * faces / d8, 2), "seconds": round(d8, 3),
           "entry_point": "KEEPFaceProcessor.process_frames_u8 (= process_image_sequence between its two ComfyUI converters)",
           "what": "uint8 frames in host memory -> batched RetinaFace pre-pass -> tracks -> device crop warp -> streamed KEEP clip loop + "
                   "ParseNet + paste-back -> uint8 frames in host memory; the product's code path with tools/synth_facehelper.py standing "
                   "in for the reference's cv2-based FaceRestoreHelper (synthetic landmarks)"}
    frames_f = frames_u8.float() / 255.0
    helper.begin_sequence()
    t0 = time.perf_counter()
    outf = proc.process_image_sequence(frames_f, 1.0, False, faces == 1, False, max_clip_length=20)
    torch.cuda.synchronize()
    df = time.perf_counter() - t0
    assert tuple(outf.shape) == (n_frames, H, W, 3) and outf.dtype == torch.float32
    rec["process_image_sequence"] = {"value": round(n_frames / df, 2), "unit": "video frames/s", "seconds": round(df, 3),
                                     "what": "the node's call: float32 RGB IMAGE tensor in host memory -> float32 IMAGE tensor in host "
                                             "memory (round 6: comfy_image_to_cv2 for the whole batch on the device -- keep_comfy_to_bgr_u8, in chunks "
                                             "under the detection pre-pass; 4x the bytes of the uint8 entry point each way)"}
    return rec


def processor_leg(net, n_crops, faces):
    """BASELINE configs[2] / [3] as the hot path sees them: `n_crops` crops stacked frame-major (`faces` crops per frame,
    interleaved: keep_processor.py:252-253) and cut into max_clip_length = 20 chunks by the processor's own code."""
    import types
    from comfyui_keep_amd.modules.keep_processor import KEEPFaceProcessor, split_clips
    # the six attributes KEEPFaceProcessor copies from a KEEPModelPack (keep_processor.py:118-124); detection / paste-back
    # are not on this leg, so no face helper (and no ComfyUI runtime) is needed
    pack = types.SimpleNamespace(keep_net=net, face_helper=None, bg_upscale_model=None, face_upscale_model=None,
                                 device=net.device, model_type_str='KEEP')
    proc = KEEPFaceProcessor(pack)
    crops = synth_crops(n_crops, seed=faces)
    proc._restore_crops_u8(crops, 20)               # warm: allocator, plan cache, batch shapes of this clip mix
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = proc._restore_crops_u8(crops, 20)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert len(out) == n_crops and out[0].shape == (512, 512, 3)
    spans = split_clips(n_crops, 20)
    return {"value": round(n_crops / dt, 3), "unit": "frames/s", "crops": n_crops, "faces_per_frame": faces,
            "clips": len(spans), "clip_lengths": sorted({e - s for s, e in spans}), "seconds": round(dt, 3),
            "what": "uint8 BGR crops in host memory -> restored uint8 BGR crops in host memory through "
                    "KEEPFaceProcessor._restore_crops_u8 (chunking, H2D, device converters, net, D2H)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--clips', type=int, default=int(os.environ.get('KEEP_BENCH_CLIPS', '48')),
                    help='independent T=20 clips per GPU per step (default 48: what 288 GB of HBM hold under the x3 policy -- BASELINE configs[3] '
                         'is 45 clips; capped by free HBM; 15 = BASELINE configs[4] per-GPU workload; 16 = the workload of rounds 1-4)')
    ap.add_argument('--precision', default=os.environ.get('KEEP_BENCH_PRECISION', 'x3'), choices=['x3', 'fp32', 'bf16'],
                    help="MFMA operand policy of `value`: x3 (split fp16, parity-grade, default), fp32 (exact f32 MFMA), "
                         "bf16 (speed policy, outside the parity tolerance)")
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='write the restored frames of the last timed step (or a fixed sample of them) to DIR/restored_frames.npy')
    ap.add_argument('--full', action='store_true',
                    help='also everything that takes runs of its own: roofline, the other policies, one clip in flight, 16 clips, '
                         'host-memory entry, configs 3 / 4 / 5, paste-back, facelib, end to end, cpu_baseline')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full without cpu_baseline')
    ap.add_argument('--cpu-baseline-frames', type=int, default=int(os.environ.get('KEEP_BENCH_CPU_T', '20')))
    ap.add_argument('--no-extras', action='store_true', help='--full with only the headline measurement + roofline (+ cpu_baseline)')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # `python bench.py --gpus N` on its own: become the launcher -- one rank per GPU under torch.distributed.run on the
        # loopback address (what the driver's own command line does).  KEEP_DIST_DEVICE=<d> puts every rank on device d
        # (a 1-GPU box: gloo wire, engine/dist.py), otherwise rank r drives GPU r over RCCL.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
               '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        sys.exit(subprocess.call(cmd, env=env))

    rank, world, local = kdist.init_from_env('gloo' if FAKE else None)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if not FAKE:
        torch.cuda.set_device(local)
    net, bcast = build_net(rank, world)
    net.set_precision(args.precision)
    B = args.clips
    if FAKE:
        x = torch.rand((B, T_CLIP, 3, 32, 32), generator=torch.Generator().manual_seed(1234 + rank))
    else:
        per_frame = {'bf16': 0.17e9, 'fp32': 0.36e9}.get(args.precision, 0.23e9)      # measured HBM per 512 x 512 frame in flight (KeepNet.clips_per_call)
        free_b, _ = torch.cuda.mem_get_info()
        if os.environ.get('KEEP_DIST_DEVICE') and world > 1:      # every rank on ONE device (1-GPU boxes): they share its HBM
            free_b //= world
        B = max(1, min(B, int(0.8 * free_b / (per_frame * T_CLIP))))
        x = synth_clip_device(T_CLIP, B, seed=1234 + rank, phase=0.37 * rank, device=torch.device('cuda', local))
    B16 = min(B, 16)                  # the side legs (other policies, policy-vs-policy comparison, host-memory entry) stay at the 16 clips of rounds 1-4

    def barrier():
        _sync()
        if world > 1:
            torch.distributed.barrier()
        _sync()

    def timed(xb, warmup, steps):
        for _ in range(warmup):
            net(xb)
        barrier()
        e0, e1 = (None, None) if FAKE else (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        t0 = time.perf_counter()
        if not FAKE:
            e0.record()
        for _ in range(steps):
            o = net(xb)
        if not FAKE:
            e1.record()
        barrier()
        d = time.perf_counter() - t0
        ev_ms = d * 1e3 if FAKE else e0.elapsed_time(e1)
        d_rank = d
        if world > 1:
            tmax = torch.tensor([d], dtype=torch.float64,
                                device='cuda' if torch.distributed.get_backend() == 'nccl' else 'cpu')
            torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
            d = float(tmax.item())
        assert torch.isfinite(o).all()
        return d, o, ev_ms, d_rank

    dt, out, ev_ms, d_rank = timed(x, args.warmup, args.steps)
    if args.dump_outputs:
        dump_outputs(out, args.dump_outputs, rank, world)
    per_rank = None
    if world > 1:
        mine = torch.tensor([B * T_CLIP * args.steps / d_rank], dtype=torch.float64,
                            device='cuda' if torch.distributed.get_backend() == 'nccl' else 'cpu')
        allr = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(allr, mine)
        per_rank = [round(float(t.item()), 2) for t in allr]

    cfg5 = None
    if world > 1 and args.full:
        # BASELINE configs[4]: one 300-crop video (15 clips x 20) per GPU through the processor's uint8 entry point, nothing
        # exchanged between ranks (shard_across_ranks off); value = all ranks' crops / slowest rank's wall time
        net.shard_across_ranks = False
        side = 8 if FAKE else 512
        u8 = [torch.randint(0, 256, (T_CLIP, side, side, 3), dtype=torch.uint8) for _ in range(15)]
        net.run_clips_u8(u8, max_b=15)
        barrier()
        t0 = time.perf_counter()
        net.run_clips_u8(u8, max_b=15)
        barrier()
        d5 = torch.tensor([time.perf_counter() - t0], dtype=torch.float64,
                          device='cuda' if torch.distributed.get_backend() == 'nccl' else 'cpu')
        torch.distributed.all_reduce(d5, op=torch.distributed.ReduceOp.MAX)
        cfg5 = {"value": round(world * 300 / float(d5.item()), 3), "unit": "frames/s", "crops_per_gpu": 300, "clips_per_gpu": 15,
                "seconds": round(float(d5.item()), 3),
                "what": "uint8 crops in host memory -> restored uint8 crops in host memory on every GPU (its own video), max over ranks"}
        del u8
    if rank == 0:
        frames = world * B * T_CLIP * args.steps
        fps = frames / dt
        line = {
            "metric": "restored 512x512 face frames/sec, T=20 clip", "value": round(fps, 3), "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 2),
            "hip_event_ms_per_step": round(ev_ms / args.steps, 2),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": DTYPE[args.precision],
            "data": "synthetic",
            "config": {"workload": f"{B} independent clips x T={T_CLIP} x 512x512 per GPU (BASELINE configs[1] clips"
                                   f"{'; 15 per GPU = configs[4]' if B == 15 else ''}), KEEP config, synthetic weights seed 0, "
                                   f"precision policy {args.precision}",
                       "clips_per_gpu": B, "clip_length": T_CLIP, "parallelism": f"dp{world} over clips",
                       "precision_policy": args.precision},
            "parity": {"x3": "split fp16 operands (3 MFMAs per product, fp32 accumulate): passes the same <= 1e-3 tests as fp32",
                       "fp32": "exact f32 MFMA: the reference arithmetic up to re-association",
                       "bf16": "operands rounded to bf16: outside the <= 1e-3 tolerance (speed policy)"}[args.precision],
            "whole_net_tflops": round(fps * FLOP_PER_FRAME_T20 / 1e12, 2),
        }
        if args.full:
            # the reference pushes every interior frame through GMFlow's CNN encoder twice (KA:979-984); the engine runs it once
            # per frame (net.py:_gmflow_clip): ~33 GFLOP per frame of the reference count are not executed here
            line["whole_net_tflops_executed"] = round(fps * (FLOP_PER_FRAME_T20 - GMFLOW_DUPLICATE_FLOP_PER_FRAME) / 1e12, 2)
        line["peak_hbm_gb"] = None if FAKE else round(torch.cuda.max_memory_allocated() / 1e9, 1)
        line["x3_range_fallbacks"] = net.x3_fallbacks
        if args.full:
            line["roofline"] = None if FAKE else conv_roofline(net, x)
        if FAKE:
            line["fake_engine"] = True          # KEEP_BENCH_FAKE_NET=1: plumbing only, not a measurement
        elif args.full:
            # ... and the 5 of 9 taps the phase form of the Upsample convolutions does not multiply (roofline.skipped_gflop_per_step)
            line["whole_net_tflops_executed"] = round(
                line["whole_net_tflops_executed"] - line["roofline"]["skipped_gflop_per_step"] * 1e9 / (dt / args.steps) / 1e12, 2)
        if world > 1:
            line["broadcast_ms"] = round(bcast["ms"], 2)
            line["broadcast_mb"] = round(bcast["mb"], 1)
            # what carried it: backend (`nccl` = RCCL over xGMI), the world size the backend saw, the library version, how many pieces
            # (<= 256 MB each) the blob went out in, and whether every rank ended up with the same bytes (exact checksum per rank)
            line["broadcast"] = dict(kdist.collective_library(), pieces=bcast.get("pieces"), largest_piece_mb=round(bcast.get("largest_piece_bytes", 0) / 1e6, 1),
                                     verified_identical_on_all_ranks=bcast["verified"])
            line["frames_per_s_per_rank"] = per_rank
            if args.full:
                line["config5_one_video_per_gpu"] = cfg5
        extras = args.full and world == 1 and not args.no_extras and not FAKE
        if extras:
            x16 = x[:B16].contiguous()
            # ---- the other policies on the same input, each compared with the exact-f32 result
            out16, aux_main = net(x16, return_aux=True)
            results = {args.precision: (out16, aux_main)}
            others = {}
            for other in [p for p in ('fp32', 'bf16', 'x3') if p != args.precision]:
                net.set_precision(other)
                d2, out2, _, _ = timed(x16, 1, 2)
                _, aux2 = net(x16, return_aux=True)
                results[other] = (out2, aux2)
                others[other] = {"value": round(B16 * T_CLIP * 2 / d2, 3), "unit": "frames/s", "clips_per_gpu": B16,
                                 "ms_per_step": round(d2 / 2 * 1e3, 2), "dtype": DTYPE[other], "roofline": conv_roofline(net, x16)}
            net.set_precision(args.precision)
            ref_out, ref_aux = results['fp32']
            for pol, (o, a) in results.items():
                if pol == 'fp32':
                    continue
                # The frame recurrence is chaotic once a single low-margin token flips (the next frame restores a different
                # prev_out), so policies are compared clip by clip up to the first frame with a differing index, and by
                # the logit margin (exact-f32 run) of the tokens that flipped there: parity means margins below ~1e-3.
                agree = (a['indices'] == ref_aux['indices'])                       # [B, T, 256]
                frame_ok = agree.flatten(2).all(2)                                  # [B, T]
                first = [next((t for t in range(T_CLIP) if not bool(frame_ok[b, t])), T_CLIP) for b in range(B16)]
                flip_margins = [float(ref_aux['margins'][b, first[b]][~agree[b, first[b]]].max()) for b in range(B16) if first[b] < T_CLIP]
                common = [(o[b, :first[b]] - ref_out[b, :first[b]]).abs().max() for b in range(B16) if first[b] > 0]
                rec = {"frame0_code_index_agreement": round(float(agree[:, 0].float().mean()), 5),
                       "frames_until_first_index_flip_per_clip": first,
                       "largest_margin_among_first_flips": (round(max(flip_margins), 6) if flip_margins else None),
                       "max_abs_pixel_diff_before_first_flip": round(float(torch.stack(common).max()), 6) if common else None,
                       "output_abs_max": round(float(ref_out.abs().max()), 3),
                       "code_index_agreement_all_frames": round(float(agree.float().mean()), 5)}
                if pol == args.precision:
                    line["vs_exact_f32_policy"] = rec
                else:
                    others[pol]["vs_exact_f32_policy"] = rec
            line["other_policies"] = others
            del results, ref_out, ref_aux
            # ---- the literal configs[1]: ONE clip in flight
            # (two warm-up passes: graph mode 'auto' runs the first occurrence of a shape eagerly and captures on the second)
            d1, _, _, _ = timed(x[:1].contiguous(), 2, 5)
            line["b1"] = {"value": round(T_CLIP * 5 / d1, 3), "unit": "frames/s", "clips_per_gpu": 1,
                          "ms_per_clip": round(d1 / 5 * 1e3, 2), "hipgraph_replay": bool(net._graphs)}
            line["config"]["one_clip_in_flight_frames_per_s"] = line["b1"]["value"]      # the literal configs[1], next to the headline
            # the same clip under the latency profile of the plans (KEEP_PLAN_REF_IMAGES=2: split-K chosen for two images per launch
            # instead of 16 -- a deployment-wide numerics setting like the precision policy, DESIGN.md section 6 "batch invariance")
            keep_ref = net.o.plan_ref_images
            net.o.plan_ref_images = 2      # (part of the plan-cache and hipGraph keys: nothing to clear)
            try:
                d1l, _, _, _ = timed(x[:1].contiguous(), 2, 5)
                line["b1"]["latency_profile"] = {"value": round(T_CLIP * 5 / d1l, 3), "unit": "frames/s", "ms_per_clip": round(d1l / 5 * 1e3, 2),
                                                 "setting": "KEEP_PLAN_REF_IMAGES=2 (keep_conv2d_args.plan_ref_images)"}
            finally:
                net.o.plan_ref_images = keep_ref
            # ---- the workload of rounds 1-4 (16 clips per call) for continuity
            d16, _, _, _ = timed(x16, 1, 2)
            line["clips16"] = {"value": round(B16 * T_CLIP * 2 / d16, 3), "unit": "frames/s", "clips_per_gpu": B16, "ms_per_step": round(d16 / 2 * 1e3, 2),
                               "what": "the same forward at the 16 clips per call rounds 1-4 were quoted on"}
            line["config"]["frames_per_s_at_16_clips_per_call"] = line["clips16"]["value"]
            # ---- the same step entered from host memory the way the processor does
            u8 = [torch.randint(0, 256, (T_CLIP, 512, 512, 3), dtype=torch.uint8).pin_memory() for _ in range(B16)]
            net.run_clips_u8(u8, max_b=B16)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = net.run_clips_u8(u8, max_b=B16)
            torch.cuda.synchronize()
            d3 = time.perf_counter() - t0
            assert len(res) == B16 and res[0].shape == (T_CLIP, 512, 512, 3)
            line["pcie_inclusive"] = {"value": round(B16 * T_CLIP / d3, 3), "unit": "frames/s", "clips_per_gpu": B16,
                                      "what": "uint8 BGR crops in pinned host memory -> restored uint8 BGR crops in host memory "
                                              "(H2D + device-side converters + net + D2H), one step"}
            del u8, res
            # ---- BASELINE configs[2] / [3] clip mixes through the processor
            line["configs"] = {"config3_300_crops_1_face": processor_leg(net, 300, 1),
                               "config4_900_crops_3_faces": processor_leg(net, 900, 3)}
            line["paste_back_gpu"] = paste_leg()
            line["facelib"] = facelib_leg()
            # ---- BASELINE configs[2] / [3] end to end: frames -> frames, every stage on the engine
            line["end_to_end"] = {"config3_300_frames_720p_1_face": pipeline_leg(net, 300, 720, 1280, 1),
                                  "config4_300_frames_1080p_3_faces": pipeline_leg(net, 300, 1080, 1920, 3)}
            # ---- the same two configurations through the product's own sequence entry point
            line["end_to_end_product"] = {"config3_300_frames_720p_1_face": product_leg(net, 300, 720, 1280, 1),
                                          "config4_300_frames_1080p_3_faces": product_leg(net, 300, 1080, 1920, 3)}
        if args.full and world == 1 and not args.no_cpu_baseline and not FAKE:
            line["cpu_baseline"] = cpu_baseline(args.cpu_baseline_frames)
        print(json.dumps(line))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
